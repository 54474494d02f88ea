// merge_plan.h -- the host arithmetic of include/tsdf_hip_merge.h (tsdf_capi.cpp, tsdf_merge.hip):
// the inverse pose and its validation, the compatibility rules of the two contexts, the search pad
// and the destination bricks a source brick's image may reach, and the scratch sizes.  Plain C++
// like esdf_plan.h, checked and sanitized on the CPU (tests/test_merge_plan.py); the candidate
// kernel evaluates merge_brick_box / merge_reaches per source brick (MERGE_FN marks them for it).
//
// The search pad.  The kernels decide validity on q, the fp32 preimage of a destination voxel's
// fp32 centre c (rule 2 of the header), and on fl(q * inv) (nearest) or fl(fl(q * inv) - 0.5f)
// (trilinear).  The candidate search works in double with the SAME fp32 matrix m, inverted exactly
// (cofactors, in double), so the only difference between the kernels' index coordinate and the
// search's is fp32 rounding, u = 2^-24 per operation:
//   c[a]    one product of the exact (float)v + 0.5f with vs                      (1 + d)
//   q[r]    three products m c, each carrying c's rounding and its own            (1 + d)^2
//           up to three additions on top of a product, two on top of m[r][3]      (1 + d)^3
//   index   the product with inv, inv = fl(1 / vs) itself, the subtraction of 0.5 (1 + d)^3
// Hence, in voxels, |index_fp32 - index_exact| <= 5 u (1 + 2e-5) (|c|_2 + |ti|_inf) / vs
// + 3 u (|q|_inf / vs + 1) + O(u^2): the rows of m have norm <= 1 + 2e-5 (the rotation rule), so
// Cauchy-Schwarz bounds sum_k |m[r][k]| |c[k]| by |c|_2.  With A = the largest |c|_2 / vs over the
// brick's image + |ti|_inf / vs + the largest |q|_inf / vs over the brick + MERGE_PAD_SLACK voxels
// (the pad's own reach and the region's extent), pad = 8 u A + 2^-10 covers it with a margin of 1.6
// and the double arithmetic of the search besides.  It grows with the coordinates: 2^-10 voxels
// near the origin, 0.02 at 4 km with 10 cm voxels, about 12 at the edge of the index domain.
//
// The candidate bricks of source brick B.  A valid sample's base voxel lies in a source brick, so
// its index coordinate lies in [8 B + off, 8 B + off + 8) per axis, off = 0 (nearest) or 0.5
// (trilinear).  That box, grown by pad, goes forward to dst (its image is a parallelepiped inside
// the bounding box of its 8 corners; growing the corners' bounding box by 2 pad >= sqrt(3) pad
// (1 + 2e-5) covers the growth).  Every destination voxel whose centre v + 0.5 lies in it is a
// candidate; their bricks, clamped to the packable range, are the box.  merge_reaches drops the
// box's corner bricks: a destination voxel centre lies within 3.5 sqrt(3) of its brick's centre
// and, when its preimage is in the grown source box, within (4 + pad) sqrt(3) (1 + 2e-5) of the
// image of that box's centre.
//
// The box is bounded.  It is empty unless the padded image meets the index domain on every axis;
// then a corner of the image has |d|_inf <= 2^23 + 2 pad + 14, so |d|_2 <= sqrt(3) (2^23 + 2 pad +
// 28) over the image, |q|_inf <= 2^23 + 9 (a brick of the source), and ti = q - m d gives
// |ti|_inf / vs <= 2^23 + 9 + (1 + 2e-5) |d|_2.  Hence A <= 5.47 * 2^23 + 7 pad + 300 and
// pad = 2^-21 A + 2^-10 < 22 voxels, whatever the pose: a non-empty box spans at most
// (8 sqrt(3) + 4 pad + 2) / 8 + 2 <= MERGE_BOX_MAX bricks per axis, 3375 candidates a source brick.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef MERGE_FN
#define MERGE_FN inline
#endif

namespace tsdf {

constexpr double MERGE_ROT_TOL = 1e-5;        // max |R R^T - I|
constexpr double MERGE_PAD_REL = 0x1p-21;     // 8 u
constexpr double MERGE_PAD_ABS = 0x1p-10;
constexpr double MERGE_PAD_SLACK = 64.0;
constexpr int32_t MERGE_BRICK_LIMIT = 1 << 20;  // packable brick coordinates: -2^20 <= b < 2^20
constexpr double MERGE_VOX_LIMIT = 8388608.0;   // the index domain: |voxel| < 2^23
constexpr int32_t MERGE_BOX_MAX = 15;           // bricks per axis of any non-empty box (below)
constexpr uint64_t MERGE_SET_MIN = 1024;      // slots of the smallest candidate set
constexpr uint64_t MERGE_MAX_PAIRS = 1ull << 31;
constexpr uint64_t MERGE_SCRATCH_FIXED = 32ull << 10;
constexpr uint64_t MERGE_SCRATCH_PER_PAIR = 48;

// The argument rules in the order they are reported; MERGE_ARG_OK passes.
enum MergeArg : int {
    MERGE_ARG_OK = 0,
    MERGE_ARG_MODE,    // not TSDF_SAMPLE_NEAREST / _TRILINEAR
    MERGE_ARG_WEIGHT,  // min_weight negative or NaN
    MERGE_ARG_POSE,    // NULL pose or a non-finite entry
    MERGE_ARG_ROT,     // max |R R^T - I| > 1e-5 or det <= 0
};

inline const char* merge_arg_text(int a) {
    switch (a) {
    case MERGE_ARG_MODE: return "mode must be TSDF_SAMPLE_NEAREST or _TRILINEAR";
    case MERGE_ARG_WEIGHT: return "min_weight is negative or NaN";
    case MERGE_ARG_POSE: return "pose is NULL or has a non-finite entry";
    case MERGE_ARG_ROT: return "pose is not a rigid transform (max |R R^T - I| > 1e-5 or det <= 0)";
    default: return nullptr;
    }
}

// The compatibility rules of the two contexts, likewise.
enum MergeCompat : int {
    MERGE_COMPAT_OK = 0,
    MERGE_COMPAT_VOXEL,  // (float)voxel_size differs in its bits
    MERGE_COMPAT_TRUNC,  // (float)sdf_trunc differs in its bits
    MERGE_COMPAT_BG,     // a Voxblox context (background 0) against a VDBFusion one (sdf_trunc)
};

inline const char* merge_compat_text(int a) {
    switch (a) {
    case MERGE_COMPAT_VOXEL: return "the contexts' voxel sizes differ";
    case MERGE_COMPAT_TRUNC: return "the contexts' truncation distances differ";
    case MERGE_COMPAT_BG: return "the contexts' backgrounds differ (Voxblox against VDBFusion)";
    default: return nullptr;
    }
}

inline uint32_t merge_float_bits(float f) {
    union { float f; uint32_t u; } v;
    v.f = f;
    return v.u;
}

// semantics: TSDF_SEM_VDBFUSION 0, TSDF_SEM_VOXBLOX 1, TSDF_SEM_VDBFUSION_F64 2
inline int merge_compat(double vs_a, double vs_b, double tau_a, double tau_b, int sem_a, int sem_b) {
    if (merge_float_bits((float)vs_a) != merge_float_bits((float)vs_b)) return MERGE_COMPAT_VOXEL;
    if (merge_float_bits((float)tau_a) != merge_float_bits((float)tau_b)) return MERGE_COMPAT_TRUNC;
    if ((sem_a == 1) != (sem_b == 1)) return MERGE_COMPAT_BG;
    return MERGE_COMPAT_OK;
}

struct MergeXform {
    float m[12];      // dst -> src, 3x4 row-major, metres: rule 1's inverse rounded to fp32
    double fwd[12];   // src -> dst in VOXELS: the exact inverse of m taken as doubles
    double ti_vox;    // max |m[r][3]| / vs
};

// Rules 1 and the pose part of the entry rules.  vs = (double)(float)voxel_size.
inline int merge_xform(const double* pose, int32_t mode, float min_weight, double vs,
                       MergeXform* X) {
    *X = MergeXform{};
    if (mode != 0 && mode != 1) return MERGE_ARG_MODE;
    if (!(min_weight >= 0.0f)) return MERGE_ARG_WEIGHT;
    if (!pose) return MERGE_ARG_POSE;
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(pose[k])) return MERGE_ARG_POSE;
    const double* P = pose;
    double dev = 0.0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double g = (P[4 * a] * P[4 * b] + P[4 * a + 1] * P[4 * b + 1]) +
                             P[4 * a + 2] * P[4 * b + 2];
            dev = std::fmax(dev, std::fabs(g - (a == b ? 1.0 : 0.0)));
        }
    const double det = P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8]) +
                       P[2] * (P[4] * P[9] - P[5] * P[8]);
    if (!(dev <= MERGE_ROT_TOL) || !(det > 0.0)) return MERGE_ARG_ROT;
    const double t0 = P[3], t1 = P[7], t2 = P[11];
    for (int r = 0; r < 3; r++) {
        const double a = P[r], b = P[4 + r], c = P[8 + r];  // row r of R^T
        X->m[4 * r] = (float)a;
        X->m[4 * r + 1] = (float)b;
        X->m[4 * r + 2] = (float)c;
        X->m[4 * r + 3] = (float)(-((a * t0 + b * t1) + c * t2));
        if (!std::isfinite(X->m[4 * r + 3])) return MERGE_ARG_POSE;  // beyond the fp32 range
    }
    // the forward map of the search: G = inverse of m's 3x3 as doubles (cofactors), in voxels
    double M[3][3], ti[3];
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) M[r][k] = (double)X->m[4 * r + k];
        ti[r] = (double)X->m[4 * r + 3];
    }
    const double dm = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) -
                      M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                      M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    double G[3][3];
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            // (cyclic indices: the cofactor's sign is built in)
            G[k][r] = (M[r1][k1] * M[r2][k2] - M[r1][k2] * M[r2][k1]) / dm;
        }
    X->ti_vox = 0.0;
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) X->fwd[4 * r + k] = G[r][k];
        // x_dst = G (q - ti) in metres; in voxels the rotation part is unchanged
        X->fwd[4 * r + 3] = -((G[r][0] * ti[0] + G[r][1] * ti[1]) + G[r][2] * ti[2]) / vs;
        X->ti_vox = std::fmax(X->ti_vox, std::fabs(ti[r]) / vs);
    }
    return MERGE_ARG_OK;
}

MERGE_FN double merge_pad(double a_vox) { return MERGE_PAD_REL * a_vox + MERGE_PAD_ABS; }

// The destination bricks source brick B may reach: lo <= D < hi per axis (an empty box where the
// image leaves the packable range), the pad, the image of the source box's centre and the squared
// reach of merge_reaches.
struct MergeBox {
    int32_t lo[3], hi[3];
    double pad, ctr[3], reach2;
};

MERGE_FN int32_t merge_clamp_brick(double b) {
    if (!(b > (double)-MERGE_BRICK_LIMIT)) return -MERGE_BRICK_LIMIT;
    if (b > (double)MERGE_BRICK_LIMIT) return MERGE_BRICK_LIMIT;
    return (int32_t)b;
}

MERGE_FN void merge_brick_box(const MergeXform& X, const int32_t B[3], int mode, MergeBox* out) {
    const double off = mode == 0 ? 0.0 : 0.5;
    double s0[3], mn[3], mx[3], cn2 = 0.0, qmax = 0.0;
    for (int a = 0; a < 3; a++) {
        s0[a] = 8.0 * (double)B[a] + off;
        qmax = fmax(qmax, fmax(fabs(s0[a]), fabs(s0[a] + 8.0)));
    }
    for (int c = 0; c < 8; c++) {
        const double s[3] = {s0[0] + ((c & 1) ? 8.0 : 0.0), s0[1] + ((c & 2) ? 8.0 : 0.0),
                             s0[2] + ((c & 4) ? 8.0 : 0.0)};
        double n2 = 0.0;
        for (int r = 0; r < 3; r++) {
            const double d = ((X.fwd[4 * r] * s[0] + X.fwd[4 * r + 1] * s[1]) +
                              X.fwd[4 * r + 2] * s[2]) + X.fwd[4 * r + 3];
            mn[r] = c == 0 ? d : fmin(mn[r], d);
            mx[r] = c == 0 ? d : fmax(mx[r], d);
            n2 += d * d;
        }
        cn2 = fmax(cn2, n2);
    }
    const double pad = merge_pad(sqrt(cn2) + X.ti_vox + qmax + MERGE_PAD_SLACK);
    out->pad = pad;
    bool empty = false;
    for (int r = 0; r < 3; r++) {
        // voxels v with mn - 2 pad <= v + 0.5 <= mx + 2 pad (floor on the low side: one more),
        // inside the index domain |v| < 2^23
        const double vlo = fmax(floor(mn[r] - 2.0 * pad - 0.5), -MERGE_VOX_LIMIT + 1.0);
        const double vhi = fmin(floor(mx[r] + 2.0 * pad - 0.5), MERGE_VOX_LIMIT - 1.0);
        empty = empty || !(vlo <= vhi);
        out->lo[r] = merge_clamp_brick(floor(vlo / 8.0));
        out->hi[r] = merge_clamp_brick(floor(vhi / 8.0) + 1.0);
        const double sc[3] = {s0[0] + 4.0, s0[1] + 4.0, s0[2] + 4.0};
        out->ctr[r] = ((X.fwd[4 * r] * sc[0] + X.fwd[4 * r + 1] * sc[1]) + X.fwd[4 * r + 2] * sc[2]) +
                      X.fwd[4 * r + 3];
    }
    // An image that leaves the domain on ONE axis reaches nothing: the box is then empty on every
    // axis, so that no loop nest over it runs through the other two (far out the pad is as wide as
    // the whole domain: a translation of 10^12 m would otherwise leave 2^42 empty iterations).
    if (empty)
        for (int r = 0; r < 3; r++) out->lo[r] = out->hi[r] = 0;
    // (4 + pad) sqrt(3) (1 + 2e-5) + 3.5 sqrt(3), rounded up
    const double reach = (8.0 + pad) * 1.7321 * 1.001 + MERGE_PAD_ABS;
    out->reach2 = reach * reach;
}

// false: no voxel of destination brick D can have its preimage in the grown source box
MERGE_FN bool merge_reaches(const MergeBox& b, int32_t dx, int32_t dy, int32_t dz) {
    const double ex = 8.0 * (double)dx + 4.0 - b.ctr[0], ey = 8.0 * (double)dy + 4.0 - b.ctr[1],
                 ez = 8.0 * (double)dz + 4.0 - b.ctr[2];
    return (ex * ex + ey * ey) + ez * ez <= b.reach2;
}

// candidate pairs of one source brick: the bricks of its box that merge_reaches keeps
MERGE_FN uint64_t merge_box_pairs(const MergeBox& b) {
    uint64_t n = 0;
    for (int32_t z = b.lo[2]; z < b.hi[2]; z++)
        for (int32_t y = b.lo[1]; y < b.hi[1]; y++)
            for (int32_t x = b.lo[0]; x < b.hi[0]; x++) n += merge_reaches(b, x, y, z) ? 1u : 0u;
    return n;
}

// The candidate set: an open-addressing table of 2^k >= 2 * pairs keys (never more than half full:
// the distinct candidates are at most the pairs), at least MERGE_SET_MIN slots.
inline uint64_t merge_set_slots(uint64_t pairs) {
    uint64_t n = MERGE_SET_MIN;
    while (n < 2 * pairs) n <<= 1;
    return n;
}

// Device scratch of one call: the set (8 B a slot, fewer than 4 * pairs slots beyond the minimum),
// the candidate list (8 B), and per candidate its flag and its pool slot (4 B each); the counters
// (MERGE_COUNTER_BYTES: two words and the flag kernel's 64 shards of a 128-byte line each).
constexpr uint64_t MERGE_COUNTER_BYTES = (16 + 64 * 16) * 8;
inline uint64_t merge_scratch_bytes(uint64_t pairs) {
    return 8 * merge_set_slots(pairs) + 16 * pairs + MERGE_COUNTER_BYTES;
}

}  // namespace tsdf
