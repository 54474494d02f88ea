// tsdf_mesh.hip — marching-cubes mesh extraction over the brick pool (SURVEY.md §8f.1;
// VDBFusion's VDBVolume::extract_triangle_mesh, restated with the oracle's semantics in
// oracle/tsdf_oracle.c tsdf_extract_mesh).
//
// One 512-lane workgroup per brick (in (z, y, x) brick order, given by the host): the brick and
// its +x / +y / +z halo — a 9^3 tile of (S, W) from up to 8 bricks, found with table lookups —
// are staged in LDS; lane l meshes the cube whose min voxel is in-brick voxel l (2 x 2 x 2 voxels,
// all observed with W >= min_weight).  Corner c is inside when S < 0; the case's triangles come
// from the generated table (tsdf_capi.cpp build_mc_table); a vertex on edge (a, b) is corner a's
// centre + t vs along the edge's axis, t = S_a / (S_a - S_b).
//   k_mesh_count  triangles per brick  -> host exclusive prefix -> offsets
//   k_mesh_emit   a block scan over the lanes' counts places every triangle: the soup is
//                 ordered by brick, then cube, then table order (the oracle's order).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_plan.h"
#include "tsdf_device.h"
#include "tsdf_ray.h"

namespace tsdf {

__constant__ uint8_t c_mc[MC_TABLES][256][32];  // per table (TSDF_MC_*): [case][0] = triangles, then 3 edge ids each
__constant__ uint8_t c_edge[12][2];  // edge -> corners (a, b), b = a | axis bit
__constant__ uint16_t c_emask[MC_TABLES][256];  // per case: the edges its triangles reference

constexpr int MESH_THREADS = 512;
constexpr int TILE = 9;

// Stage the 9^3 tile of brick `key`: s_ok[t] = observed (W > 0, W >= min_weight).  A neighbour is
// looked up in the halo (H, HP) first -- bricks another rank owns after a border reduce, of which
// this context may hold a reset copy -- then in the context's own table; the brick itself only in
// the own table.
__device__ void mesh_tile(const Table& T, const Pool& Pl, const Table& H, const Pool& HP,
                          uint64_t key, float min_weight, float* s_S, uint8_t* s_ok,
                          uint32_t* s_slot) {
    const int bx = (int)(key & 0x1FFFFFu) - BRICK_COORD_BIAS;
    const int by = (int)((key >> 21) & 0x1FFFFFu) - BRICK_COORD_BIAS;
    const int bz = (int)((key >> 42) & 0x1FFFFFu) - BRICK_COORD_BIAS;
    if (threadIdx.x < 8) {  // the brick and its 7 +x/+y/+z neighbours
        const int dx = threadIdx.x & 1, dy = (threadIdx.x >> 1) & 1, dz = threadIdx.x >> 2;
        uint32_t slot = INVALID_SLOT, src = 0u;
        const int nx = bx + dx, ny = by + dy, nz = bz + dz;
        if (nx < BRICK_COORD_BIAS && ny < BRICK_COORD_BIAS && nz < BRICK_COORD_BIAS) {
            const uint64_t nk = pack_brick(nx, ny, nz);
            // the brick itself always from the own table: a reset copy of a brick owned elsewhere
            // is meshed by its owner (its halo copy would mesh its cubes twice)
            if (H.keys && threadIdx.x != 0) {
                const int64_t h = table_find(H, nk);
                if (h >= 0) {
                    slot = H.slots[h];
                    src = 1u << 31;
                }
            }
            if (!src) {
                const int64_t h = table_find(T, nk);
                if (h >= 0) slot = T.slots[h];
            }
        }
        // bit 31: a halo slot (slots are < 2^31 in both pools)
        s_slot[threadIdx.x] = slot < T.max_bricks || src ? slot | src : INVALID_SLOT;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TILE * TILE * TILE; t += MESH_THREADS) {
        const int tx = t % TILE, ty = (t / TILE) % TILE, tz = t / (TILE * TILE);
        const uint32_t ss = s_slot[(tx >> 3) | ((ty >> 3) << 1) | ((tz >> 3) << 2)];
        const bool halo = ss != INVALID_SLOT && (ss >> 31);
        const uint32_t slot = ss & 0x7FFFFFFFu;
        const Pool& P = halo ? HP : Pl;
        float S = 0.0f;
        uint8_t ok = 0;
        if (ss != INVALID_SLOT && slot < (halo ? H.max_bricks : T.max_bricks)) {
            const size_t i = (size_t)slot * BRICK_VOX + ((tz & 7) << 6) + ((ty & 7) << 3) + (tx & 7);
            const float W = P.weight[i];
            S = P.sdf[i];
            ok = (W > 0.0f && W >= min_weight) ? 1 : 0;
        }
        s_S[t] = S;
        s_ok[t] = ok;
    }
    __syncthreads();
}

// The cube of in-brick voxel l: case index, or -1 when a corner is unobserved.
__device__ __forceinline__ int mesh_case(const float* s_S, const uint8_t* s_ok, int l, float S[8]) {
    const int x = l & 7, y = (l >> 3) & 7, z = l >> 6;
    int k = 0;
    for (int q = 0; q < 8; q++) {
        const int t = (x + (q & 1)) + TILE * ((y + ((q >> 1) & 1)) + TILE * (z + (q >> 2)));
        if (!s_ok[t]) return -1;
        S[q] = s_S[t];
        k |= (S[q] < 0.0f ? 1 : 0) << q;
    }
    return k;
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_count(Table T, Pool Pl, Table H, Pool HP,
                                                            const uint64_t* __restrict__ keys,
                                                            uint32_t nb, float min_weight,
                                                            uint32_t* __restrict__ counts, int tab) {
    __shared__ float s_S[TILE * TILE * TILE];
    __shared__ uint8_t s_ok[TILE * TILE * TILE];
    __shared__ uint32_t s_slot[8];
    __shared__ uint32_t s_sum;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        if (threadIdx.x == 0) s_sum = 0u;
        mesh_tile(T, Pl, H, HP, keys[b], min_weight, s_S, s_ok, s_slot);
        float S[8];
        const int k = mesh_case(s_S, s_ok, threadIdx.x, S);
        const uint32_t nt = k >= 0 ? c_mc[tab][k][0] : 0u;
        const uint32_t w = wave_sum<uint32_t>(nt);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&s_sum, w);
        __syncthreads();
        if (threadIdx.x == 0) counts[b] = s_sum;
        __syncthreads();
    }
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_emit(Table T, Pool Pl, Table H, Pool HP,
                                                           const uint64_t* __restrict__ keys,
                                                           uint32_t nb, float min_weight, float vs,
                                                           const uint64_t* __restrict__ offsets, int tab,
                                                           float* __restrict__ tri) {
    __shared__ float s_S[TILE * TILE * TILE];
    __shared__ uint8_t s_ok[TILE * TILE * TILE];
    __shared__ uint32_t s_slot[8];
    __shared__ uint32_t s_w[MESH_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint64_t key = keys[b];
        mesh_tile(T, Pl, H, HP, key, min_weight, s_S, s_ok, s_slot);
        float S[8];
        const int l = threadIdx.x;
        const int k = mesh_case(s_S, s_ok, l, S);
        const uint32_t nt = k >= 0 ? c_mc[tab][k][0] : 0u;
        // exclusive scan of the lanes' triangle counts (cube order)
        const uint32_t incl = wave_incl_scan(nt);
        if (lane == 63) s_w[wid] = incl;
        __syncthreads();
        uint32_t off = 0;
        for (int q = 0; q < wid; q++) off += s_w[q];
        __syncthreads();  // s_w and the tile are reused by the next brick
        if (nt) {
            const int bx = (int)(key & 0x1FFFFFu) - BRICK_COORD_BIAS;
            const int by = (int)((key >> 21) & 0x1FFFFFu) - BRICK_COORD_BIAS;
            const int bz = (int)((key >> 42) & 0x1FFFFFu) - BRICK_COORD_BIAS;
            const int x = bx * 8 + (l & 7), y = by * 8 + ((l >> 3) & 7), z = bz * 8 + (l >> 6);
            float* out = tri + 9 * (offsets[b] + off + incl - nt);
            for (uint32_t t = 0; t < nt; t++) {
                for (int j = 0; j < 3; j++) {
                    const int ed = c_mc[tab][k][1 + 3 * t + j];
                    const int a = c_edge[ed][0], bb = c_edge[ed][1];
                    const int ax = (a ^ bb) == 1 ? 0 : ((a ^ bb) == 2 ? 1 : 2);
                    const float tt = S[a] / (S[a] - S[bb]);
                    float p0 = ((float)(x + (a & 1)) + 0.5f) * vs;
                    float p1 = ((float)(y + ((a >> 1) & 1)) + 0.5f) * vs;
                    float p2 = ((float)(z + ((a >> 2) & 1)) + 0.5f) * vs;
                    if (ax == 0) p0 = p0 + tt * vs;
                    else if (ax == 1) p1 = p1 + tt * vs;
                    else p2 = p2 + tt * vs;
                    out[9 * t + 3 * j] = p0;
                    out[9 * t + 3 * j + 1] = p1;
                    out[9 * t + 3 * j + 2] = p2;
                }
            }
        }
    }
}

// ---- indexed mesh (include/tsdf_hip_mesh.h): shared vertices, normals, a voxel box --------------
//
// The listed bricks (keys, sorted in (z, y, x) order: the box's bricks and, one voxel past its high
// side, the owners of their vertices) each have a 1536-bit vertex mask, bit 3 l + axis for the edge
// from in-brick voxel l along axis.  An edge belongs to the brick of its min voxel: for a cube of
// brick b that is b or one of its seven +x / +y / +z neighbours.
//   k_mesh_slot_index  pool slot -> position in the list: the tile's 8 slots name the owners
//   k_mesh_mark      cubes OR their triangles' edges into the owners' masks; triangles per brick
//   k_mesh_vcount    popcount of each mask            -> host exclusive prefixes (mesh_plan.h)
//   k_mesh_vertices  an 11^3 tile of (S, observed) per brick; every set bit writes its position and
//                    normal at vbase + its rank in the mask
//   k_mesh_indices   the cubes again: three indices per triangle, vbase[owner] + rank, at the
//                    soup's triangle offset
// Integer ORs and popcounts only: the result does not depend on thread or pool order.

constexpr int VMASK = MESH_VMASK_WORDS;
constexpr uint32_t NO_BRICK = 0xFFFFFFFFu;
constexpr int VTILE = 11;  // in-brick coordinates -1 .. 9

// The list position of the neighbour at +d of the brick whose tile mesh_tile staged (s_slot: the
// 8 pool slots; d = dx | dy << 1 | dz << 2, d != 0), NO_BRICK when it is not held or not listed.
__device__ __forceinline__ uint32_t mesh_owner(const uint32_t* s_slot, int d,
                                               const uint32_t* __restrict__ slot_idx,
                                               uint32_t n_pool) {
    const uint32_t slot = s_slot[d];
    return slot < n_pool ? slot_idx[slot] : NO_BRICK;
}

// slot_idx[pool slot] = the brick's position in the sorted list (the caller fills it with NO_BRICK)
__global__ __launch_bounds__(256) void k_mesh_slot_index(Table T, const uint64_t* __restrict__ keys,
                                                        uint32_t nb, uint32_t n_pool,
                                                        uint32_t* __restrict__ slot_idx) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const int64_t h = table_find(T, keys[i]);
        if (h < 0) continue;
        const uint32_t slot = T.slots[h];
        if (slot < n_pool) slot_idx[slot] = (uint32_t)i;
    }
}

// The cube of lane l of brick `key`, as mesh_case, restricted to the box: -1 outside.
__device__ __forceinline__ int mesh_case_box(const float* s_S, const uint8_t* s_ok, int l,
                                             uint64_t key, const MeshBox& B, float S[8]) {
    const int x = ((int)(key & 0x1FFFFFu) - BRICK_COORD_BIAS) * 8 + (l & 7);
    const int y = ((int)((key >> 21) & 0x1FFFFFu) - BRICK_COORD_BIAS) * 8 + ((l >> 3) & 7);
    const int z = ((int)((key >> 42) & 0x1FFFFFu) - BRICK_COORD_BIAS) * 8 + (l >> 6);
    if (x < B.lo[0] || x >= B.hi[0] || y < B.lo[1] || y >= B.hi[1] || z < B.lo[2] || z >= B.hi[2])
        return -1;
    return mesh_case(s_S, s_ok, l, S);
}

// Edge ed of the cube of in-brick voxel l: its owner d among the 8 bricks and its mask bit.
__device__ __forceinline__ void mesh_edge_bit(int l, int ed, int& d, int& bit) {
    const int a = c_edge[ed][0], bb = c_edge[ed][1];
    const int ax = (a ^ bb) == 1 ? 0 : ((a ^ bb) == 2 ? 1 : 2);
    const int px = (l & 7) + (a & 1), py = ((l >> 3) & 7) + ((a >> 1) & 1);
    const int pz = (l >> 6) + ((a >> 2) & 1);
    d = (px >> 3) | ((py >> 3) << 1) | ((pz >> 3) << 2);
    bit = 3 * (((pz & 7) << 6) | ((py & 7) << 3) | (px & 7)) + ax;
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_mark(Table T, Pool Pl,
                                                           const uint64_t* __restrict__ keys,
                                                           uint32_t nb, float min_weight, int tab,
                                                           MeshBox B,
                                                           const uint32_t* __restrict__ slot_idx,
                                                           uint32_t n_pool,
                                                           uint32_t* __restrict__ mask,
                                                           uint32_t* __restrict__ tcnt) {
    __shared__ float s_S[TILE * TILE * TILE];
    __shared__ uint8_t s_ok[TILE * TILE * TILE];
    __shared__ uint32_t s_slot[8];
    __shared__ uint32_t s_m[VMASK];
    __shared__ uint32_t s_sum;
    const Table H{};  // no halo: the context holds the whole field
    const Pool HP{};
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint64_t key = keys[b];
        if (threadIdx.x < VMASK) s_m[threadIdx.x] = 0u;
        if (threadIdx.x == 0) s_sum = 0u;
        mesh_tile(T, Pl, H, HP, key, min_weight, s_S, s_ok, s_slot);
        float S[8];
        const int l = threadIdx.x;
        const int k = mesh_case_box(s_S, s_ok, l, key, B, S);
        const uint32_t nt = k >= 0 ? c_mc[tab][k][0] : 0u;
        if (nt) {
            // the edges the case's triangles reference, one at a time
            for (uint32_t em = c_emask[tab][k]; em; em &= em - 1u) {
                const int ed = __ffs((int)em) - 1;
                int d, bit;
                mesh_edge_bit(l, ed, d, bit);
                const uint32_t m = 1u << (bit & 31);
                if (d == 0) {
                    atomicOr(&s_m[bit >> 5], m);
                } else {
                    // (held and listed: both ends of the edge are observed)
                    const uint32_t o = mesh_owner(s_slot, d, slot_idx, n_pool);
                    if (o < nb) atomicOr(&mask[(size_t)o * VMASK + (bit >> 5)], m);
                }
            }
        }
        const uint32_t w = wave_sum<uint32_t>(nt);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&s_sum, w);
        __syncthreads();
        if (threadIdx.x < VMASK && s_m[threadIdx.x])
            atomicOr(&mask[(size_t)b * VMASK + threadIdx.x], s_m[threadIdx.x]);
        if (threadIdx.x == 0) tcnt[b] = s_sum;
        __syncthreads();
    }
}

// One wave per brick: the set bits of its mask.
__global__ __launch_bounds__(256) void k_mesh_vcount(const uint32_t* __restrict__ mask, uint32_t nb,
                                                    uint32_t* __restrict__ vcnt) {
    const int lane = threadIdx.x & 63;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nb;
         b += (uint64_t)gridDim.x * 4) {
        const uint32_t n = lane < VMASK ? (uint32_t)__popc(mask[b * VMASK + lane]) : 0u;
        const uint32_t s = wave_sum<uint32_t>(n);
        if (lane == 0) vcnt[b] = s;
    }
}

// g_j(v) of include/tsdf_hip_mesh.h rule 3 at tile position t, `stride` the axis' tile stride.
__device__ __forceinline__ float mesh_grad(const float* s_S, const uint8_t* s_ok, int t, int stride,
                                           float inv) {
    const bool op = s_ok[t + stride], om = s_ok[t - stride];
    if (op && om) return (s_S[t + stride] - s_S[t - stride]) * (0.5f * inv);
    if (op) return (s_S[t + stride] - s_S[t]) * inv;
    if (om) return (s_S[t] - s_S[t - stride]) * inv;
    return 0.0f;
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_vertices(
    Table T, Pool Pl, const uint64_t* __restrict__ keys, uint32_t nb, float min_weight, float vs,
    float inv, const uint32_t* __restrict__ mask, const uint32_t* __restrict__ vcnt,
    const uint32_t* __restrict__ vbase, float* __restrict__ vert, float* __restrict__ nrm) {
    __shared__ float s_S[VTILE * VTILE * VTILE];
    __shared__ uint8_t s_ok[VTILE * VTILE * VTILE];
    __shared__ uint32_t s_slot[27];
    __shared__ uint32_t s_m[VMASK];
    __shared__ uint32_t s_pre[VMASK];
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        if (vcnt[b] == 0u) continue;  // (the whole workgroup)
        const uint64_t key = keys[b];
        const int bx = (int)(key & 0x1FFFFFu) - BRICK_COORD_BIAS;
        const int by = (int)((key >> 21) & 0x1FFFFFu) - BRICK_COORD_BIAS;
        const int bz = (int)((key >> 42) & 0x1FFFFFu) - BRICK_COORD_BIAS;
        if (threadIdx.x < 27) {  // the brick and its 26 neighbours
            const int nx = bx + (int)(threadIdx.x % 3) - 1;
            const int ny = by + (int)((threadIdx.x / 3) % 3) - 1;
            const int nz = bz + (int)(threadIdx.x / 9) - 1;
            uint32_t slot = INVALID_SLOT;
            if (nx >= -BRICK_COORD_BIAS && nx < BRICK_COORD_BIAS && ny >= -BRICK_COORD_BIAS &&
                ny < BRICK_COORD_BIAS && nz >= -BRICK_COORD_BIAS && nz < BRICK_COORD_BIAS) {
                const int64_t h = table_find(T, pack_brick(nx, ny, nz));
                if (h >= 0) slot = T.slots[h];
            }
            s_slot[threadIdx.x] = slot < T.max_bricks ? slot : INVALID_SLOT;
        } else if (threadIdx.x >= 64 && threadIdx.x < 64 + VMASK) {
            s_m[threadIdx.x - 64] = mask[(size_t)b * VMASK + (threadIdx.x - 64)];
        }
        __syncthreads();
        for (int t = threadIdx.x; t < VTILE * VTILE * VTILE; t += MESH_THREADS) {
            const int cx = t % VTILE - 1, cy = (t / VTILE) % VTILE - 1;
            const int cz = t / (VTILE * VTILE) - 1;
            const uint32_t slot =
                s_slot[((cx + 8) >> 3) + 3 * ((cy + 8) >> 3) + 9 * ((cz + 8) >> 3)];
            float S = 0.0f;
            uint8_t ok = 0;
            if (slot != INVALID_SLOT) {
                const size_t i =
                    (size_t)slot * BRICK_VOX + ((cz & 7) << 6) + ((cy & 7) << 3) + (cx & 7);
                const float W = Pl.weight[i];
                S = Pl.sdf[i];
                ok = (W > 0.0f && W >= min_weight) ? 1 : 0;
            }
            s_S[t] = S;
            s_ok[t] = ok;
        }
        if (threadIdx.x < VMASK) {  // vertices before word w
            uint32_t p = 0u;
            for (int q = 0; q < (int)threadIdx.x; q++) p += (uint32_t)__popc(s_m[q]);
            s_pre[threadIdx.x] = p;
        }
        __syncthreads();
        const int l = threadIdx.x;
        const int lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
        const int ta = (lx + 1) + VTILE * ((ly + 1) + VTILE * (lz + 1));
        const size_t v0 = vbase[b];
        for (int ax = 0; ax < 3; ax++) {
            const int bit = 3 * l + ax;
            const uint32_t w = s_m[bit >> 5];
            if (!((w >> (bit & 31)) & 1u)) continue;
            const size_t v = v0 + s_pre[bit >> 5] + (uint32_t)__popc(w & ((1u << (bit & 31)) - 1u));
            const int st = ax == 0 ? 1 : (ax == 1 ? VTILE : VTILE * VTILE);
            const int tb = ta + st;
            const float tt = s_S[ta] / (s_S[ta] - s_S[tb]);
            float p0 = ((float)(bx * 8 + lx) + 0.5f) * vs;
            float p1 = ((float)(by * 8 + ly) + 0.5f) * vs;
            float p2 = ((float)(bz * 8 + lz) + 0.5f) * vs;
            if (ax == 0) p0 = p0 + tt * vs;
            else if (ax == 1) p1 = p1 + tt * vs;
            else p2 = p2 + tt * vs;
            vert[3 * v] = p0;
            vert[3 * v + 1] = p1;
            vert[3 * v + 2] = p2;
            if (nrm) {
                float g[3];
                for (int j = 0; j < 3; j++) {
                    const int sj = j == 0 ? 1 : (j == 1 ? VTILE : VTILE * VTILE);
                    const float ga = mesh_grad(s_S, s_ok, ta, sj, inv);
                    const float gb = mesh_grad(s_S, s_ok, tb, sj, inv);
                    g[j] = ga + tt * (gb - ga);
                }
                const float n2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
                float n0 = 0.0f, n1 = 0.0f, n2v = 0.0f;
                if (n2 > 0.0f) {
                    const float len = sqrtf(n2);
                    n0 = g[0] / len;
                    n1 = g[1] / len;
                    n2v = g[2] / len;
                }
                nrm[3 * v] = n0;
                nrm[3 * v + 1] = n1;
                nrm[3 * v + 2] = n2v;
            }
        }
        __syncthreads();  // the tile and the mask are reused by the next brick
    }
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_indices(
    Table T, Pool Pl, const uint64_t* __restrict__ keys, uint32_t nb, float min_weight, int tab,
    MeshBox B, const uint32_t* __restrict__ slot_idx, uint32_t n_pool,
    const uint32_t* __restrict__ mask, const uint32_t* __restrict__ tcnt,
    const uint64_t* __restrict__ toff, const uint32_t* __restrict__ vbase,
    uint32_t* __restrict__ tri) {
    __shared__ float s_S[TILE * TILE * TILE];
    __shared__ uint8_t s_ok[TILE * TILE * TILE];
    __shared__ uint32_t s_slot[8];
    __shared__ uint32_t s_vb[8];
    __shared__ uint32_t s_m[8 * VMASK];    // the 8 owners' masks
    __shared__ uint32_t s_pre[8 * VMASK];  // and, per word, the owner's vertices before it
    __shared__ uint32_t s_w[MESH_THREADS / 64];
    const Table H{};
    const Pool HP{};
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        if (tcnt[b] == 0u) continue;  // (the whole workgroup)
        const uint64_t key = keys[b];
        mesh_tile(T, Pl, H, HP, key, min_weight, s_S, s_ok, s_slot);
        if (threadIdx.x < 8 * VMASK) {  // the 8 owners' masks and, below, their first vertices
            const int d = threadIdx.x / VMASK;
            const uint32_t o = d ? mesh_owner(s_slot, d, slot_idx, n_pool) : b;
            s_m[threadIdx.x] = o < nb ? mask[(size_t)o * VMASK + threadIdx.x % VMASK] : 0u;
            if (threadIdx.x % VMASK == 0) s_vb[d] = o < nb ? vbase[o] : 0u;
        }
        float S[8];
        const int l = threadIdx.x;
        const int k = mesh_case_box(s_S, s_ok, l, key, B, S);
        const uint32_t nt = k >= 0 ? c_mc[tab][k][0] : 0u;
        const uint32_t incl = wave_incl_scan(nt);
        if (lane == 63) s_w[wid] = incl;
        __syncthreads();
        if (threadIdx.x < 8 * VMASK) {
            uint32_t p = 0u;
            for (int q = (int)(threadIdx.x / VMASK) * VMASK; q < (int)threadIdx.x; q++)
                p += (uint32_t)__popc(s_m[q]);
            s_pre[threadIdx.x] = p;
        }
        uint32_t off = 0;
        for (int q = 0; q < wid; q++) off += s_w[q];
        __syncthreads();
        if (nt) {
            uint32_t* out = tri + 3 * (toff[b] + off + incl - nt);
            for (uint32_t i = 0; i < 3 * nt; i++) {
                int d, bit;
                mesh_edge_bit(l, c_mc[tab][k][1 + i], d, bit);
                const int wi = d * VMASK + (bit >> 5);
                out[i] = s_vb[d] + s_pre[wi] + (uint32_t)__popc(s_m[wi] & ((1u << (bit & 31)) - 1u));
            }
        }
        __syncthreads();  // the tile, the masks and s_w are reused by the next brick
    }
}

hipError_t upload_mc_table(const uint8_t tab[MC_TABLES][256][32], const uint8_t edge[12][2]) {
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_mc), tab, MC_TABLES * 256 * 32);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_edge), edge, 12 * 2);
    uint16_t em[MC_TABLES][256];
    for (int t = 0; t < MC_TABLES; t++)
        for (int k = 0; k < 256; k++) {
            em[t][k] = 0;
            for (int i = 0; i < 3 * tab[t][k][0]; i++) em[t][k] |= (uint16_t)(1u << tab[t][k][1 + i]);
        }
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_emask), em, sizeof em);
    return e;
}

hipError_t launch_mesh_count(const Table& T, const Pool& Pl, const Table& H, const Pool& HP,
                             const uint64_t* d_keys, uint32_t nb, float min_weight, int tab,
                             uint32_t* d_counts, hipStream_t st) {
    if (nb == 0) return hipSuccess;
    const uint32_t grid = nb < 4096u ? nb : 4096u;
    k_mesh_count<<<grid, MESH_THREADS, 0, st>>>(T, Pl, H, HP, d_keys, nb, min_weight, d_counts,
                                                tab);
    return hipGetLastError();
}

hipError_t launch_mesh_emit(const Table& T, const Pool& Pl, const Table& H, const Pool& HP,
                            const uint64_t* d_keys, uint32_t nb, float min_weight, int tab,
                            float vs, const uint64_t* d_offsets, float* d_tri, hipStream_t st) {
    if (nb == 0) return hipSuccess;
    const uint32_t grid = nb < 4096u ? nb : 4096u;
    k_mesh_emit<<<grid, MESH_THREADS, 0, st>>>(T, Pl, H, HP, d_keys, nb, min_weight, vs,
                                               d_offsets, tab, d_tri);
    return hipGetLastError();
}

hipError_t launch_mesh_mark(const Table& T, const Pool& Pl, const uint64_t* d_keys, uint32_t nb,
                            float min_weight, int tab, const MeshBox& B, uint32_t n_pool,
                            uint32_t* d_slot_idx, uint32_t* d_mask, uint32_t* d_tcnt,
                            uint32_t* d_vcnt, hipStream_t st) {
    if (nb == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_mask, 0, (size_t)nb * VMASK * sizeof(uint32_t), st);
    // (every byte 0xFF: NO_BRICK)
    if (e == hipSuccess) e = hipMemsetAsync(d_slot_idx, 0xFF, (size_t)n_pool * 4, st);
    if (e != hipSuccess) return e;
    const uint32_t ig = (nb + 255u) / 256u;
    k_mesh_slot_index<<<ig < 4096u ? ig : 4096u, 256, 0, st>>>(T, d_keys, nb, n_pool,
                                                               d_slot_idx);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t grid = nb < 4096u ? nb : 4096u;
    k_mesh_mark<<<grid, MESH_THREADS, 0, st>>>(T, Pl, d_keys, nb, min_weight, tab, B, d_slot_idx,
                                               n_pool, d_mask, d_tcnt);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t waves = (nb + 3u) / 4u;
    k_mesh_vcount<<<waves < 4096u ? waves : 4096u, 256, 0, st>>>(d_mask, nb, d_vcnt);
    return hipGetLastError();
}

hipError_t launch_mesh_fill(const Table& T, const Pool& Pl, const uint64_t* d_keys, uint32_t nb,
                            float min_weight, int tab, const MeshBox& B, float vs, float inv,
                            uint32_t n_pool, const uint32_t* d_slot_idx, const uint32_t* d_mask,
                            const uint32_t* d_tcnt, const uint32_t* d_vcnt,
                            const uint64_t* d_toff, const uint32_t* d_vbase, float* d_vert,
                            float* d_nrm, uint32_t* d_tri, hipStream_t st) {
    if (nb == 0) return hipSuccess;
    const uint32_t grid = nb < 4096u ? nb : 4096u;
    k_mesh_vertices<<<grid, MESH_THREADS, 0, st>>>(T, Pl, d_keys, nb, min_weight, vs, inv, d_mask,
                                                   d_vcnt, d_vbase, d_vert, d_nrm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_mesh_indices<<<grid, MESH_THREADS, 0, st>>>(T, Pl, d_keys, nb, min_weight, tab, B,
                                                  d_slot_idx, n_pool, d_mask, d_tcnt, d_toff,
                                                  d_vbase, d_tri);
    return hipGetLastError();
}

}  // namespace tsdf
