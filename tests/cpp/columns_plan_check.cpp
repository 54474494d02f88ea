// The host arithmetic of the column maps (noetic-slam_amd/csrc/columns_plan.h) on the CPU: answers
// the queries on stdin, one per line, for tests/test_columns_plan.py to compare with its Python
// restatement over a grid:
//   A <lo x3> <hi x3> <occ_band> <min_weight> <min_occ> <min_free>   (int64 x6, floats as %a, u32 x2)
//        -> "<rule> <nx> <ny> <nz> <cells> <bx0> <by0> <bz0> <nbx> <nby> <nbz> <cols>" of
//           columns_check
//   G <cols>            -> "<groups> <grid> <trips>"
//   M <cols> <nbx> <bx0> <by0> <trip> <wg> <wave>
//        -> "<index> <bx> <by>" of the brick column of that wave ("<index> - -" past the last)
//   C <cols>            -> "<visited> <min visits> <max visits>" over every (trip, wg, wave) of the
//                          launch: each brick column exactly once means "<cols> 1 1"
// and prints "ok <queries>" at the end.  Built plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../noetic-slam_amd/csrc/columns_plan.h"

using namespace tsdf;

int main() {
    char line[512];
    unsigned long long n_q = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == 'A') {
            int64_t lo[3], hi[3];
            float band, min_w;
            uint32_t min_occ, min_free;
            if (std::sscanf(line + 1, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64
                                      " %" SCNd64 " %a %a %" SCNu32 " %" SCNu32,
                            &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2], &band, &min_w, &min_occ,
                            &min_free) != 10)
                return 2;
            ColBox B;
            const int rule = columns_check(lo, hi, band, min_w, min_occ, min_free, &B);
            if ((rule == COL_ARG_OK) != (columns_arg_text(rule) == nullptr)) return 3;
            std::printf("%d %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 " %" PRId64 " %" PRId64
                        " %" PRId64 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n",
                        rule, B.n[0], B.n[1], B.n[2], B.cells, B.b0[0], B.b0[1], B.b0[2], B.nb[0],
                        B.nb[1], B.nb[2], B.cols);
        } else if (line[0] == 'G') {
            uint64_t cols;
            if (std::sscanf(line + 1, "%" SCNu64, &cols) != 1) return 2;
            std::printf("%" PRIu64 " %" PRIu32 " %" PRIu64 "\n", col_groups(cols), col_grid(cols),
                        col_trips(cols));
        } else if (line[0] == 'M') {
            uint64_t cols, trip;
            uint32_t nbx, wg, wave;
            int64_t bx0, by0;
            if (std::sscanf(line + 1, "%" SCNu64 " %" SCNu32 " %" SCNd64 " %" SCNd64 " %" SCNu64
                                      " %" SCNu32 " %" SCNu32,
                            &cols, &nbx, &bx0, &by0, &trip, &wg, &wave) != 7)
                return 2;
            const uint64_t c = col_index(trip, wg, wave, col_grid(cols));
            if (c < cols)
                std::printf("%" PRIu64 " %" PRId64 " %" PRId64 "\n", c, col_bx(bx0, nbx, c),
                            col_by(by0, nbx, c));
            else
                std::printf("%" PRIu64 " - -\n", c);
        } else if (line[0] == 'C') {
            uint64_t cols;
            if (std::sscanf(line + 1, "%" SCNu64, &cols) != 1) return 2;
            std::vector<uint8_t> seen(cols, 0);
            const uint32_t grid = col_grid(cols);
            uint64_t visited = 0;
            for (uint64_t trip = 0; trip < col_trips(cols); trip++)
                for (uint32_t wg = 0; wg < grid; wg++) {
                    if (trip * grid + wg >= col_groups(cols)) continue;  // the kernel's loop bound
                    for (uint32_t wave = 0; wave < COL_WAVES; wave++) {
                        const uint64_t c = col_index(trip, wg, wave, grid);
                        if (c >= cols) continue;
                        if (seen[c] < 255) seen[c]++;
                        visited++;
                    }
                }
            unsigned mn = 255, mx = 0;
            for (uint8_t s : seen) {
                mn = s < mn ? s : mn;
                mx = s > mx ? s : mx;
            }
            if (!cols) mn = mx = 0;
            std::printf("%" PRIu64 " %u %u\n", visited, mn, mx);
        } else {
            return 2;
        }
        n_q++;
    }
    std::printf("ok %llu\n", n_q);
    return 0;
}
