// Check of the walk kernels' ray-tile map and its column detector (noetic-slam_amd/csrc/ray_tile.h)
// on the CPU:
//   * the map: for H in {0, 64, 96, 128, 256} and scans of n points -- empty, one point, below one
//     group, exactly one and three groups, groups plus a remainder that is and is not a multiple of
//     1024 -- the (block, slot) pairs whose point is below n are a bijection onto [0, n): every
//     point exactly once; every block holds at most 1024 points; there are ceil(n / 1024) blocks;
//     a full group's block bt holds exactly the points g 32 H + c H + 32 bt + b (c, b < 32); each
//     half of a tile is 32 columns x 16 beams; 16 consecutive slots are 16 consecutive points;
//     H = 0 and every block past the last full group are the identity (slot s = point 1024 b + s);
//   * the detector: synthetic spinning-sensor grids (beams falling or rising in elevation, origin
//     off zero) of 64 x 64 and 128 x 40 are accepted with their H, a 256-beam one with 256, and a
//     64-beam grid is not taken for a 128-beam one; rejected: a grid with one point dropped, a
//     grid with one point dropped and one appended (n % H == 0 again), a shuffled cloud,
//     n % H != 0, a single column, a 32-beam sensor, a cloud with a NaN at a boundary.
// Exits non-zero on the first misses.  Built plain and with -fsanitize=address,undefined
// (tests/test_ray_tile.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../noetic-slam_amd/csrc/ray_tile.h"

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

static void check_map(uint32_t n, uint32_t H) {
    CHECK(tile_height_ok(H), "H %u not accepted", H);
    const uint32_t nb = (n + TILE_RAYS - 1) / TILE_RAYS;
    std::vector<uint32_t> seen(n, 0u);
    const uint32_t G = 32 * H, full = H ? n / G : 0;  // full groups
    for (uint32_t b = 0; b < nb; b++) {
        const TileBlock tb = tile_block(n, H, b);
        const bool tiled = H != 0 && b < full * (H / 32);
        CHECK((tb.H != 0) == tiled, "n %u H %u block %u: tiled %d, expected %d", n, H, b, tb.H != 0,
              tiled);
        uint32_t held = 0;
        for (uint32_t s = 0; s < TILE_RAYS; s++) {
            const uint32_t p = tile_point(tb, s);
            if (p >= n) {
                CHECK(!tiled, "n %u H %u block %u slot %u: a tile's slot is empty", n, H, b, s);
                continue;
            }
            held++;
            seen[p]++;
            if (!tiled) {
                CHECK(p == b * TILE_RAYS + s, "n %u H %u block %u slot %u: %u is not consecutive", n,
                      H, b, s, p);
            } else {
                const uint32_t g = b / (H / 32), bt = b % (H / 32), r = p - g * G;
                const uint32_t c = r / H, bm = r % H;
                CHECK(p >= g * G && c < 32 && bm >= 32 * bt && bm < 32 * bt + 32,
                      "n %u H %u block %u slot %u: point %u outside the tile", n, H, b, s, p);
                // a half is 32 columns x 16 beams, beams fast
                CHECK((bm - 32 * bt) / 16 == s / 512 && c == (s % 512) / 16 && bm % 16 == s % 16,
                      "n %u H %u block %u slot %u: point %u (column %u beam %u) breaks the half layout",
                      n, H, b, s, p, c, bm);
            }
        }
        CHECK(held <= TILE_RAYS && held == std::min(TILE_RAYS, n - b * TILE_RAYS),
              "n %u H %u block %u holds %u points", n, H, b, held);
    }
    for (uint32_t p = 0; p < n; p++)
        CHECK(seen[p] == 1, "n %u H %u: point %u mapped %u times", n, H, p, seen[p]);
    // past the scan's blocks (k_count's paired workgroups ask): consecutive, so every slot is empty
    const TileBlock past = tile_block(n, H, nb);
    CHECK(past.H == 0 && past.base >= n, "n %u H %u: the block past the end holds points", n, H);
}

// A spinning sensor at `o`: beams of elevation +-22 degrees (falling with the beam index when
// `falling`), columns stepping in azimuth, ranges varying per point; column-major.
static std::vector<float> grid(uint32_t H, uint32_t W, bool falling, const float o[3],
                               uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> range(2.0f, 30.0f);
    std::vector<float> xyz;
    for (uint32_t c = 0; c < W; c++)
        for (uint32_t b = 0; b < H; b++) {
            const double f = (double)b / (H - 1), el = (falling ? 1 - 2 * f : 2 * f - 1) * 0.39;
            const double az = -6.283185307179586 * c / W, r = range(rng);
            xyz.push_back((float)(o[0] + r * std::cos(el) * std::cos(az)));
            xyz.push_back((float)(o[1] + r * std::cos(el) * std::sin(az)));
            xyz.push_back((float)(o[2] + r * std::sin(el)));
        }
    return xyz;
}

static uint32_t detect(const std::vector<float>& xyz, const float o[3]) {
    return tile_detect(xyz.data(), (uint32_t)(xyz.size() / 3), o[0], o[1], o[2]);
}

static void check_detect() {
    const float o[3] = {8.0f, -3.5f, 0.25f};
    CHECK(detect(grid(64, 64, true, o, 1), o) == 64, "64 x 64 (falling) not accepted as 64");
    CHECK(detect(grid(64, 64, false, o, 2), o) == 64, "64 x 64 (rising) not accepted as 64");
    CHECK(detect(grid(128, 40, true, o, 3), o) == 128, "128 x 40 not accepted as 128");
    CHECK(detect(grid(256, 8, false, o, 4), o) == 256, "256 x 8 not accepted as 256");
    CHECK(detect(grid(32, 64, true, o, 5), o) == 0, "a 32-beam sensor accepted");
    CHECK(detect(grid(128, 1, true, o, 6), o) == 0, "a single column accepted");
    {
        std::vector<float> g = grid(64, 64, true, o, 7);
        g.erase(g.begin() + 3 * 1000, g.begin() + 3 * 1001);  // one point dropped: n % 64 != 0
        CHECK(detect(g, o) == 0, "a grid with a point dropped accepted");
        g.insert(g.end(), {o[0] + 5.0f, o[1], o[2] - 1.0f});  // n % 64 == 0 again, columns shifted
        CHECK(detect(g, o) == 0, "a grid with a point dropped and one appended accepted");
    }
    {
        std::vector<float> g = grid(128, 40, true, o, 8);
        g.resize(g.size() - 3 * 5);
        CHECK(detect(g, o) == 0, "n %% H != 0 accepted");
    }
    {
        const std::vector<float> g = grid(128, 40, true, o, 9);
        std::vector<uint32_t> perm(g.size() / 3);
        for (uint32_t i = 0; i < perm.size(); i++) perm[i] = i;
        std::shuffle(perm.begin(), perm.end(), std::mt19937(10));
        std::vector<float> sh;
        for (uint32_t i : perm) sh.insert(sh.end(), g.begin() + 3 * i, g.begin() + 3 * i + 3);
        CHECK(detect(sh, o) == 0, "a shuffled cloud accepted");
    }
    {
        std::vector<float> g = grid(64, 64, true, o, 11);
        g[3 * 64 * 17 + 2] = NAN;  // the first point of column 17
        CHECK(detect(g, o) == 0, "a NaN at a column boundary accepted");
    }
}

int main() {
    const uint32_t hs[] = {0, 64, 96, 128, 256};
    for (uint32_t H : hs) {
        const uint32_t G = H ? 32 * H : 4096;
        const uint32_t ns[] = {0, 1, 1023, 1024, G - 1, G, G + 1, G + 1024, G + 1500, 3 * G,
                               3 * G + 777, 3 * G + 1024};
        for (uint32_t n : ns) check_map(n, H);
    }
    check_map(131072, 128);  // a 128 x 1024 scan: 32 groups, no remainder
    if (tile_height_ok(32) || tile_height_ok(100) || tile_height_ok(288)) {
        std::printf("a column height outside the map's accepted\n");
        fails++;
    }
    check_detect();
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
