// The host arithmetic of the distance field (noetic-slam_amd/csrc/esdf_plan.h) on the CPU: answers
// the queries on stdin, one per line, for tests/test_esdf_plan.py to compare with its Python
// restatement over a grid:
//   A <lo x3> <hi x3> <radius> <site_band> <min_weight>   (int64 x6, u32, floats as %a)
//        -> "<rule> <nx> <ny> <nz> <total>" of esdf_check
//   T <radius> <nx> <ny> <nz>
//        -> "<seg> <hx> <hy> <hz> <lds x> <lds y> <lds z> <tiles x> <tiles y> <tiles z> <grid x>
//            <scratch bytes>"
// and prints "ok <queries>" at the end.  Built plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../noetic-slam_amd/csrc/esdf_plan.h"

using namespace tsdf;

int main() {
    char line[512];
    unsigned long long n_q = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == 'A') {
            int64_t lo[3], hi[3];
            uint32_t radius;
            float band, min_w;
            if (std::sscanf(line + 1, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64
                                      " %" SCNd64 " %" SCNu32 " %a %a",
                            &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2], &radius, &band,
                            &min_w) != 9)
                return 2;
            EsdfBox B;
            const int rule = esdf_check(lo, hi, radius, band, min_w, &B);
            if ((rule == ESDF_ARG_OK) != (esdf_arg_text(rule) == nullptr)) return 3;
            std::printf("%d %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n", rule, B.n[0], B.n[1],
                        B.n[2], B.total);
        } else if (line[0] == 'T') {
            uint32_t radius;
            EsdfBox B{};
            if (std::sscanf(line + 1, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &radius,
                            &B.n[0], &B.n[1], &B.n[2]) != 4)
                return 2;
            B.total = (uint64_t)B.n[0] * B.n[1] * B.n[2];
            const uint32_t hx = esdf_halo(radius, B.n[0]), hy = esdf_halo(radius, B.n[1]),
                           hz = esdf_halo(radius, B.n[2]);
            const uint64_t tx = esdf_tiles_x(B);
            std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32
                        " %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu32 " %" PRIu64 "\n",
                        esdf_seg(radius), hx, hy, hz, esdf_lds_x(hx), esdf_lds_axis(radius, hy),
                        esdf_lds_axis(radius, hz), tx,
                        esdf_tiles_axis(radius, B.n[0], B.n[1], B.n[2]),
                        esdf_tiles_axis(radius, (uint64_t)B.n[0] * B.n[1], B.n[2], 1),
                        esdf_grid(tx), esdf_scratch_bytes(B.total));
        } else {
            return 2;
        }
        n_q++;
    }
    std::printf("ok %llu\n", n_q);
    return 0;
}
