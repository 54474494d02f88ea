// Check of the host brick-key codec (noetic-slam_amd/csrc/brick_key.h) on the CPU, against naive
// restatements:
//   * pack / coordinate round trip at the range corners (-2^20, -1, 0, 2^20 - 1 on every axis) and
//     on 4096 random triples, against a restatement with multiplications;
//   * the (z, y, x) order against comparison of the signed (z, y, x) tuples: random pairs, and
//     pairs equal on one or two axes;
//   * the range rule at both ends;
//   * brick_halo_needed against a set-based restatement: random sets of at most 64 bricks in a 4^3
//     box, the empty set, one brick, a full 2^3 block (its outer +shell: 19 bricks) and bricks at
//     2^20 - 1 on one, two and three axes (no neighbour past the range); sorted and unique.
// Exits non-zero on the first miss.  Built plain and with -fsanitize=address,undefined
// (tests/test_brick_key.py).
#include <array>
#include <cstdio>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "../../noetic-slam_amd/csrc/brick_key.h"

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

using Brick = std::array<int32_t, 3>;
constexpr int32_t LO = -(1 << 20), HI = (1 << 20) - 1;

// the key by arithmetic: sum of (b + 2^20) * 2^(21 axis)
static uint64_t naive_key(const Brick& b) {
    uint64_t k = 0, scale = 1;
    for (int a = 0; a < 3; a++, scale *= 2097152ull) k += (uint64_t)((int64_t)b[a] + 1048576) * scale;
    return k;
}

static void check_round_trip(std::mt19937_64& rng) {
    const int32_t corner[4] = {LO, -1, 0, HI};
    std::vector<Brick> bricks;
    for (int i = 0; i < 64; i++) bricks.push_back({corner[i & 3], corner[(i >> 2) & 3], corner[i >> 4]});
    std::uniform_int_distribution<int32_t> any(LO, HI);
    for (int i = 0; i < 4096; i++) bricks.push_back({any(rng), any(rng), any(rng)});
    for (const Brick& b : bricks) {
        const uint64_t k = brick_key_pack(b[0], b[1], b[2]);
        CHECK(k == naive_key(b), "pack(%d, %d, %d) = %llx", b[0], b[1], b[2], (unsigned long long)k);
        CHECK(k < (1ull << 63), "pack(%d, %d, %d) sets bit 63", b[0], b[1], b[2]);
        for (int a = 0; a < 3; a++)
            CHECK(brick_key_coord(k, a) == b[a], "coord(pack(%d, %d, %d), %d) = %d", b[0], b[1], b[2],
                  a, brick_key_coord(k, a));
    }
}

static void check_order(std::mt19937_64& rng) {
    // a small range (many ties per axis) and the whole one
    for (const int32_t span : {2, HI}) {
        std::uniform_int_distribution<int32_t> any(span == HI ? LO : -span, span);
        for (int i = 0; i < 20000; i++) {
            Brick p = {any(rng), any(rng), any(rng)}, q = {any(rng), any(rng), any(rng)};
            const int same = i % 8;  // axes forced equal: none, one, two or all three
            for (int a = 0; a < 3; a++)
                if ((same >> a) & 1) q[a] = p[a];
            const bool want = std::make_tuple(p[2], p[1], p[0]) < std::make_tuple(q[2], q[1], q[0]);
            const bool got = brick_key_less_zyx(brick_key_pack(p[0], p[1], p[2]),
                                                brick_key_pack(q[0], q[1], q[2]));
            CHECK(got == want, "order of (%d, %d, %d) and (%d, %d, %d): %d", p[0], p[1], p[2], q[0],
                  q[1], q[2], (int)got);
        }
    }
}

static void check_range() {
    CHECK(brick_coord_ok(LO) && brick_coord_ok(HI) && brick_coord_ok(0) && brick_coord_ok(-1),
          "range rule refuses a coordinate inside");
    CHECK(!brick_coord_ok(LO - 1) && !brick_coord_ok(HI + 1), "range rule takes a coordinate outside");
    CHECK(!brick_coord_ok(INT32_MIN) && !brick_coord_ok(INT32_MAX), "range rule takes an int32 end");
}

// the halo of a set of bricks, with sets of coordinates
static std::vector<uint64_t> naive_halo(const std::vector<Brick>& bricks) {
    const std::set<Brick> have(bricks.begin(), bricks.end());
    std::set<uint64_t> need;
    for (const Brick& b : have)
        for (int dz = 0; dz < 2; dz++)
            for (int dy = 0; dy < 2; dy++)
                for (int dx = 0; dx < 2; dx++) {
                    const Brick q = {b[0] + dx, b[1] + dy, b[2] + dz};
                    if (q[0] > HI || q[1] > HI || q[2] > HI || have.count(q)) continue;
                    need.insert(naive_key(q));
                }
    return std::vector<uint64_t>(need.begin(), need.end());
}

static void check_halo_of(const std::vector<Brick>& bricks, const char* what, long expect = -1) {
    std::vector<uint64_t> have;
    for (const Brick& b : bricks) have.push_back(brick_key_pack(b[0], b[1], b[2]));
    std::sort(have.begin(), have.end());
    have.erase(std::unique(have.begin(), have.end()), have.end());
    const std::vector<uint64_t> got = brick_halo_needed(have);
    CHECK(got == naive_halo(bricks), "halo of %s differs (%zu keys)", what, got.size());
    for (size_t i = 1; i < got.size(); i++)
        CHECK(got[i - 1] < got[i], "halo of %s is not sorted and unique at %zu", what, i);
    if (expect >= 0) CHECK((long)got.size() == expect, "halo of %s: %zu keys", what, got.size());
}

static void check_halo(std::mt19937_64& rng) {
    check_halo_of({}, "the empty set", 0);
    check_halo_of({{3, -2, 7}}, "one brick", 7);
    check_halo_of({{LO, LO, LO}}, "the lowest brick", 7);
    std::vector<Brick> block;
    for (int i = 0; i < 8; i++) block.push_back({-1 + (i & 1), 5 + ((i >> 1) & 1), LO + (i >> 2)});
    check_halo_of(block, "a 2^3 block", 27 - 8);
    check_halo_of({{HI, 0, 0}}, "a brick at the top of x", 3);
    check_halo_of({{0, HI, 0}}, "a brick at the top of y", 3);
    check_halo_of({{0, 0, HI}}, "a brick at the top of z", 3);
    check_halo_of({{HI, HI, 0}}, "a brick at the top of x and y", 1);
    check_halo_of({{HI, HI, HI}}, "the highest brick", 0);
    check_halo_of({{HI, HI, HI}, {HI - 1, HI, HI}, {HI, HI - 1, HI - 1}}, "bricks around the top");
    std::uniform_int_distribution<int32_t> cell(0, 3), count(1, 64);
    const Brick base[3] = {{-2, -2, -2}, {HI - 3, HI - 3, HI - 3}, {LO, 100, HI - 3}};
    for (int i = 0; i < 300; i++) {
        std::vector<Brick> bricks(count(rng));
        const Brick& o = base[i % 3];
        for (Brick& b : bricks) b = {o[0] + cell(rng), o[1] + cell(rng), o[2] + cell(rng)};
        check_halo_of(bricks, "a random set");
    }
}

int main() {
    std::mt19937_64 rng(20240521);
    check_round_trip(rng);
    check_order(rng);
    check_range();
    check_halo(rng);
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
