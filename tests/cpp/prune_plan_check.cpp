// The host arithmetic of prune and evict (noetic-slam_amd/csrc/prune_plan.h) on the CPU: answers
// the queries on stdin, one per line, for tests/test_prune_plan.py to compare with its Python
// restatement over a grid:
//   B <c> <r> <vs>                 (doubles, %a)  -> "<lo> <hi>" of cube_box_axis
//   P <arrays>                                   -> "<bricks per piece>" of evict_piece_bricks
// and prints "ok <queries>" at the end.  Built plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../noetic-slam_amd/csrc/prune_plan.h"

using namespace tsdf;

int main() {
    char line[512];
    unsigned long long n_q = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == 'B') {
            double c, r, vs;
            if (std::sscanf(line + 1, "%la %la %la", &c, &r, &vs) != 3) return 2;
            int32_t lo, hi;
            cube_box_axis(c, r, vs, &lo, &hi);
            std::printf("%d %d\n", lo, hi);
        } else if (line[0] == 'P') {
            int arrays;
            if (std::sscanf(line + 1, "%d", &arrays) != 1) return 2;
            std::printf("%" PRIu64 "\n", evict_piece_bricks(arrays));
        } else {
            return 2;
        }
        n_q++;
    }
    std::printf("ok %llu\n", n_q);
    return 0;
}
