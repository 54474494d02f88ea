// The host arithmetic of the frontier voxels (noetic-slam_amd/csrc/frontier_plan.h) on the CPU:
// answers the queries on stdin, one per line, for tests/test_frontier_plan.py to compare with its
// Python restatement:
//   A <box> <lo x3> <hi x3> <free_band> <min_weight> <connectivity> <min_unknown>
//        (box: 0 none, 1 lo only, 2 hi only, 3 both; int64 x6; floats as %a; int32 x2)
//        -> "<rule> <empty> <lo x3> <hi x3>" of frontier_check (the clamped box; zeros when a
//           rule is broken) and, on a second line, the rule's text ("-" when none is broken)
//   O    -> the 26 offsets, "<dx> <dy> <dz>" each, on one line
//   G <bricks>          -> "<grid>" of frontier_grid
//   P <n> <counts ...>  -> "<n_voxels> <n_frontier_bricks> <sum> <offsets ...>" of frontier_prefix
//                          and frontier_sum
//   K <bx> <by> <bz> <lo x3> <hi x3>   -> "<0|1>": mesh_brick_in_box(key, B, 0) of that box
// and prints "ok <queries>" at the end.  Built plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../noetic-slam_amd/csrc/frontier_plan.h"

using namespace tsdf;

int main() {
    static char line[1 << 16];
    unsigned long long n_q = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == 'A') {
            int box;
            int64_t lo[3], hi[3];
            float band, min_w;
            int32_t conn, min_unknown;
            if (std::sscanf(line + 1, "%d %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64
                                      " %" SCNd64 " %a %a %" SCNd32 " %" SCNd32,
                            &box, &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2], &band, &min_w,
                            &conn, &min_unknown) != 11)
                return 2;
            MeshBox B;
            bool empty = false;
            const int rule = frontier_check(box & 1 ? lo : nullptr, box & 2 ? hi : nullptr, band,
                                            min_w, conn, min_unknown, &B, &empty);
            const char* text = frontier_arg_text(rule);
            if ((rule == FRONTIER_ARG_OK) != (text == nullptr)) return 3;
            if (rule != FRONTIER_ARG_OK)
                std::printf("%d 0 0 0 0 0 0 0\n%s\n", rule, text);
            else
                std::printf("%d %d %d %d %d %d %d %d\n-\n", rule, empty ? 1 : 0, B.lo[0], B.lo[1],
                            B.lo[2], B.hi[0], B.hi[1], B.hi[2]);
        } else if (line[0] == 'O') {
            for (int k = 0; k < FRONTIER_OFFSETS; k++)
                std::printf("%d %d %d%s", FRONTIER_OFFSET.d[k][0], FRONTIER_OFFSET.d[k][1],
                            FRONTIER_OFFSET.d[k][2], k + 1 < FRONTIER_OFFSETS ? " " : "\n");
        } else if (line[0] == 'G') {
            uint64_t nb;
            if (std::sscanf(line + 1, "%" SCNu64, &nb) != 1) return 2;
            std::printf("%" PRIu32 "\n", frontier_grid(nb));
        } else if (line[0] == 'P') {
            char* p = line + 1;
            const uint64_t n = std::strtoull(p, &p, 10);
            std::vector<uint32_t> cnt(n);
            for (uint64_t i = 0; i < n; i++) cnt[i] = (uint32_t)std::strtoull(p, &p, 10);
            std::vector<uint64_t> off(n);
            uint64_t nv = 0, nfb = 0;
            frontier_prefix(cnt.data(), n, off.data(), &nv, &nfb);
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64, nv, nfb, frontier_sum(cnt.data(), n));
            for (uint64_t o : off) std::printf(" %" PRIu64, o);
            std::printf("\n");
        } else if (line[0] == 'K') {
            int32_t b[3];
            int64_t lo[3], hi[3];
            if (std::sscanf(line + 1, "%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd64 " %" SCNd64
                                      " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64,
                            &b[0], &b[1], &b[2], &lo[0], &lo[1], &lo[2], &hi[0], &hi[1],
                            &hi[2]) != 9)
                return 2;
            MeshBox B;
            bool empty = false;
            if (frontier_check(lo, hi, 0.0f, 0.0f, 6, 1, &B, &empty) != FRONTIER_ARG_OK) return 4;
            std::printf("%d\n", !empty && mesh_brick_in_box(brick_key_pack(b[0], b[1], b[2]), B, 0)
                                    ? 1 : 0);
        } else {
            return 2;
        }
        n_q++;
    }
    std::printf("ok %llu\n", n_q);
    return 0;
}
