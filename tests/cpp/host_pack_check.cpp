// Check of the host input helpers (noetic-slam_amd/csrc/host_pack.h) on the CPU:
//   * pack_xyz against a naive per-field restatement, bit for bit: six record layouts, each also
//     one byte off alignment, clouds of 0 / 1 / 7 / 1000 points with NaN, +-inf, denormals, -0 and
//     doubles beyond the float range, packed whole and as 1 / 3 / 8 parts through run_parts on real
//     PackPools (one case with a pool-less context);
//   * pack_shares: three destinations with shares [floor(k n / 3), floor((k + 1) n / 3)) and parts
//     that straddle the share boundaries, also n = 2 (an empty share);
//   * sector_of_angle against a brute-force restatement of in_sector's wrap rule: N = 2, 3, 8,
//     every rotation, a at / just below / just above every start, at 0, just below 4 and NaN;
//     exactly one sector claims each non-NaN a.
// Exits non-zero on the first miss.  Built plain and with -fsanitize=address,undefined
// (tests/test_host_pack.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../noetic-slam_amd/csrc/host_pack.h"

using namespace tsdf;

static int fails = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            if (++fails > 10) return;     \
        }                                 \
    } while (0)

// ---- test clouds ---------------------------------------------------------------------------------

static double special(uint64_t i) {
    const double inf = std::numeric_limits<double>::infinity();
    const double v[] = {std::nan(""), inf, -inf, -0.0, 0.0, 1e-42 /* a float denormal */, -3e-45,
                        4.9e-324 /* a double denormal */, 1e300, -1e300, 3.5e38 /* > FLT_MAX */,
                        (double)std::numeric_limits<float>::max(), 1.0 + 1e-12, -7.25, 16777217.0};
    return v[i % (sizeof v / sizeof v[0])];
}

// coordinate a of point i: specials mixed with ordinary values
static double coord(uint64_t i, int a) {
    const uint64_t j = 3 * i + (uint64_t)a;
    if (j % 5 == 0) return special(j / 5);
    return ((double)(int64_t)(j * 2654435761u % 200003) - 100001.0) * 1.0009765625e-3;
}

struct Cloud {
    std::vector<char> bytes;  // one spare byte in front: base = data() + misalign
    RecordView v;
    uint64_t n;
};

static Cloud make_cloud(uint64_t n, uint32_t step, uint32_t off, bool f64, int misalign) {
    Cloud c;
    c.n = n;
    c.bytes.assign(n * step + 1, (char)0xA5);
    char* base = c.bytes.data() + misalign;
    for (uint64_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            const double d = coord(i, a);
            if (f64) {
                std::memcpy(base + i * step + off + 8 * a, &d, 8);
            } else {
                const float f = (float)d;  // (beyond the float range: +-inf, as stored by a caller)
                std::memcpy(base + i * step + off + 4 * a, &f, 4);
            }
        }
    c.v = RecordView{base, step, off, f64};
    return c;
}

// the naive restatement: field by field, no fast path
static std::vector<float> naive(const Cloud& c) {
    std::vector<float> out(3 * c.n);
    for (uint64_t i = 0; i < c.n; i++)
        for (int a = 0; a < 3; a++) {
            const char* q = c.v.base + i * c.v.point_step + c.v.xyz_offset;
            if (c.v.is_f64) {
                double d;
                std::memcpy(&d, q + 8 * a, 8);
                out[3 * i + a] = (float)d;
            } else {
                std::memcpy(&out[3 * i + a], q + 4 * a, 4);
            }
        }
    return out;
}

static bool same_bits(const float* a, const float* b, uint64_t words) {
    return words == 0 || std::memcmp(a, b, words * 4) == 0;
}

// ---- pack_xyz, run_parts ---------------------------------------------------------------------------

struct PoolSet {
    const char* name;
    std::vector<PackPool*> pools;
    int parts;  // with a large cloud
};

static void check_pack(const std::vector<PoolSet>& sets) {
    struct L { uint32_t step, off; bool f64; };
    const L layouts[] = {{12, 0, false}, {32, 0, false}, {32, 4, false}, {48, 16, false},
                         {24, 0, true},  {40, 8, true}};
    const uint64_t counts[] = {0, 1, 7, 1000};
    for (const L& l : layouts)
        for (int mis = 0; mis < 2; mis++)
            for (uint64_t n : counts) {
                const Cloud c = make_cloud(n, l.step, l.off, l.f64, mis);
                CHECK(c.v.layout_ok(), "layout_ok false for step %u off %u", l.step, l.off);
                const std::vector<float> ref = naive(c);
                std::vector<float> got(3 * n + 3, -1.0f);
                pack_xyz(c.v, 0, n, got.data());
                CHECK(same_bits(got.data(), ref.data(), 3 * n) && got[3 * n] == -1.0f,
                      "pack_xyz whole: step %u off %u f64 %d mis %d n %llu", l.step, l.off, l.f64,
                      mis, (unsigned long long)n);
                // a sub-range packs to the front of its destination
                if (n >= 7) {
                    std::fill(got.begin(), got.end(), -1.0f);
                    pack_xyz(c.v, 2, 6, got.data());
                    CHECK(same_bits(got.data(), ref.data() + 6, 12) && got[12] == -1.0f,
                          "pack_xyz range: step %u off %u f64 %d mis %d", l.step, l.off, l.f64, mis);
                }
                // as parts through run_parts on real pools (min_points 0: these small clouds would
                // otherwise be one part; the threshold itself: check_run_parts)
                for (const PoolSet& s : sets) {
                    std::fill(got.begin(), got.end(), -1.0f);
                    std::vector<std::atomic<int>> hits(s.parts);
                    for (auto& h : hits) h.store(0);
                    const int parts = run_parts(
                        s.pools.data(), (uint32_t)s.pools.size(), n,
                        [&](int q, uint64_t i0, uint64_t i1) {
                            hits[q].fetch_add(1);
                            pack_xyz(c.v, i0, i1, got.data() + 3 * i0);
                        },
                        0);
                    bool once = parts == s.parts;
                    for (auto& h : hits) once = once && h.load() == 1;
                    CHECK(once && same_bits(got.data(), ref.data(), 3 * n) && got[3 * n] == -1.0f,
                          "pack_xyz %s: step %u off %u f64 %d mis %d n %llu", s.name, l.step, l.off,
                          l.f64, mis, (unsigned long long)n);
                }
            }
    // layout_ok is the one statement of the rule
    CHECK(!(RecordView{nullptr, 11, 0, false}.layout_ok()), "step 11 fp32 accepted");
    CHECK(!(RecordView{nullptr, 32, 21, false}.layout_ok()), "offset 21 of 32 fp32 accepted");
    CHECK((RecordView{nullptr, 32, 20, false}.layout_ok()), "offset 20 of 32 fp32 refused");
    CHECK(!(RecordView{nullptr, 23, 0, true}.layout_ok()), "step 23 fp64 accepted");
    CHECK(!(RecordView{nullptr, 40, 17, true}.layout_ok()), "offset 17 of 40 fp64 accepted");
    CHECK((RecordView{nullptr, 40, 16, true}.layout_ok()), "offset 16 of 40 fp64 refused");
    CHECK(!(RecordView{nullptr, 0, 0xFFFFFFF8u, false}.layout_ok()), "wrapping offset accepted");
}

// run_parts itself: every part once, the ranges tile [0, n) in order, the count is part_count's,
// and the packed cloud is the naive one -- above and below the single-part threshold
static void check_run_parts(const std::vector<PoolSet>& sets) {
    const uint64_t counts[] = {0, 1, 7, 1000, PARTS_MIN_POINTS - 1, PARTS_MIN_POINTS, 40001};
    for (const PoolSet& s : sets)
        for (uint64_t n : counts)
            for (int f64 = 0; f64 < 2; f64++) {
                const Cloud c = make_cloud(n, f64 ? 40 : 32, f64 ? 8 : 4, f64 != 0, 1);
                const std::vector<float> ref = naive(c);
                std::vector<float> got(3 * n + 3, -1.0f);
                const int want = n >= PARTS_MIN_POINTS ? s.parts : 1;
                std::vector<uint64_t> lo(want + 1, ~0ull), hi(want + 1, ~0ull);
                std::vector<std::atomic<int>> hits(want + 1);
                for (auto& h : hits) h.store(0);
                const int parts = run_parts(
                    s.pools.data(), (uint32_t)s.pools.size(), n, [&](int q, uint64_t i0, uint64_t i1) {
                        if (q < 0 || q >= want) q = want;  // a part that must not exist
                        hits[q].fetch_add(1);
                        lo[q] = i0;
                        hi[q] = i1;
                        pack_xyz(c.v, i0, i1, got.data() + 3 * i0);
                    });
                bool ok = parts == want && hits[want].load() == 0 &&
                          parts == part_count(s.pools.data(), (uint32_t)s.pools.size(), n);
                for (int q = 0; q < want && ok; q++)
                    ok = hits[q].load() == 1 && lo[q] == (q ? hi[q - 1] : 0) && lo[q] <= hi[q];
                ok = ok && hi[want - 1] == n;
                CHECK(ok && same_bits(got.data(), ref.data(), 3 * n) && got[3 * n] == -1.0f,
                      "run_parts %s: n %llu f64 %d gave %d parts, want %d", s.name,
                      (unsigned long long)n, f64, parts, want);
            }
}

// ---- pack_shares -----------------------------------------------------------------------------------

static void check_shares() {
    for (uint64_t n : {(uint64_t)0, (uint64_t)2, (uint64_t)7, (uint64_t)1000})
        for (int f64 = 0; f64 < 2; f64++)
            for (uint64_t parts : {(uint64_t)1, (uint64_t)2, (uint64_t)5, (uint64_t)8}) {
                const Cloud c = make_cloud(n, f64 ? 24 : 12, 0, f64 != 0, 0);  // (12: the memcpy path)
                const std::vector<float> ref = naive(c);
                uint64_t lo[4];
                for (uint64_t k = 0; k <= 3; k++) lo[k] = n * k / 3;
                std::vector<float> buf[3];
                float* dst[3];
                for (int k = 0; k < 3; k++) {
                    buf[k].assign(3 * (lo[k + 1] - lo[k]) + 3, -1.0f);
                    dst[k] = buf[k].data();
                }
                // 2, 5 and 8 parts over 3 shares: parts straddle the share boundaries
                for (uint64_t q = 0; q < parts; q++)
                    pack_shares(c.v, n * q / parts, n * (q + 1) / parts, lo, 3, dst);
                for (int k = 0; k < 3; k++) {
                    const uint64_t m = lo[k + 1] - lo[k];
                    CHECK(same_bits(dst[k], ref.data() + 3 * lo[k], 3 * m) && dst[k][3 * m] == -1.0f,
                          "pack_shares: n %llu f64 %d parts %llu share %d", (unsigned long long)n,
                          f64, (unsigned long long)parts, k);
                }
            }
}

// ---- sector_of_angle -------------------------------------------------------------------------------

// in_sector (tsdf_device.h) on sector k's bounds [lo, hi), hi = the next sector's start
static bool in_sector_ref(float a, float lo, float hi) {
    const bool wrap = hi <= lo;
    return wrap ? (a >= lo || a < hi) : (a >= lo && a < hi);
}

static void check_sectors() {
    for (uint32_t N : {2u, 3u, 8u})
        for (uint32_t r0 = 0; r0 < N; r0++)
            for (int first_zero = 0; first_zero < 2; first_zero++) {
                // ascending starts in [0, 4); sector (r0 + j) mod N starts at u[j]
                float u[8], start[8];
                for (uint32_t j = 0; j < N; j++)
                    u[j] = first_zero && j == 0 ? 0.0f : 0.37f + 3.6f * (float)j / (float)N;
                for (uint32_t j = 0; j < N; j++) start[(r0 + j) % N] = u[j];
                std::vector<float> as = {0.0f, std::nextafterf(4.0f, 0.0f)};
                for (uint32_t j = 0; j < N; j++) {
                    as.push_back(u[j]);
                    as.push_back(std::nextafterf(u[j], 5.0f));
                    if (u[j] > 0.0f) as.push_back(std::nextafterf(u[j], -1.0f));
                }
                for (float a : as) {
                    const int got = sector_of_angle(a, u, r0, N);
                    int claims = 0, who = -1;
                    for (uint32_t k = 0; k < N; k++)
                        if (in_sector_ref(a, start[k], start[(k + 1) % N])) {
                            claims++;
                            who = (int)k;
                        }
                    CHECK(claims == 1 && got == who,
                          "sector_of_angle: N %u r0 %u a %.9g gave %d, in_sector %d (%d claims)", N,
                          r0, (double)a, got, who, claims);
                }
                CHECK(sector_of_angle(std::nanf(""), u, r0, N) == -1, "NaN got a sector (N %u)", N);
            }
}

int main() {
    PackPool a(3), b(2), c(4), one(0);
    const std::vector<PoolSet> sets = {
        {"1 part (no pool)", {nullptr}, 1},
        {"1 part (a pool without workers)", {&one}, 1},
        {"3 parts", {&b}, 3},
        {"8 parts", {&a, &c}, 8},
        {"8 parts, a pool-less context between", {&a, nullptr, &c}, 8},
        {"5 parts, context 0 pool-less", {nullptr, &c}, 5},
    };
    check_pack(sets);
    check_run_parts(sets);
    check_shares();
    check_sectors();
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
