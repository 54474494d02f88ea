// The host arithmetic of the map merge (noetic-slam_amd/csrc/merge_plan.h) on the CPU: answers the
// queries on stdin, one per line, for tests/test_merge_plan.py to compare with its Python
// restatement (floats as %a):
//   X <pose x12> <mode> <min_weight> <vs>        -> "<rule> <m x12> <fwd x12> <ti_vox>" of merge_xform
//   X0 <mode> <min_weight> <vs>                  -> the same for a NULL pose
//   C <vs a> <vs b> <tau a> <tau b> <sem a> <sem b>  -> "<rule>" of merge_compat
//   B <pose x12> <vs> <mode> <bx> <by> <bz>      -> "<lo x3> <hi x3> <pad> <pairs>" of merge_brick_box
//   S <pairs>                                    -> "<set slots> <scratch bytes>"
// and prints "ok <queries>" at the end.  Built plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../noetic-slam_amd/csrc/merge_plan.h"

using namespace tsdf;

static bool doubles(char** p, double* out, int n) {
    for (int k = 0; k < n; k++) {
        char* end = nullptr;
        out[k] = std::strtod(*p, &end);
        if (end == *p) return false;
        *p = end;
    }
    return true;
}

static void print_xform(int rule, const MergeXform& X) {
    std::printf("%d", rule);
    for (int k = 0; k < 12; k++) std::printf(" %a", (double)X.m[k]);
    for (int k = 0; k < 12; k++) std::printf(" %a", X.fwd[k]);
    std::printf(" %a\n", X.ti_vox);
}

int main() {
    char line[2048];
    unsigned long long n_q = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        char* p = line + 1;
        if (line[0] == 'X' && line[1] == '0') {
            double a[3];
            p = line + 2;
            if (!doubles(&p, a, 3)) return 2;
            MergeXform X;
            const int rule = merge_xform(nullptr, (int32_t)a[0], (float)a[1], a[2], &X);
            if ((rule == MERGE_ARG_OK) != (merge_arg_text(rule) == nullptr)) return 3;
            print_xform(rule, X);
        } else if (line[0] == 'X') {
            double a[15];
            if (!doubles(&p, a, 15)) return 2;
            MergeXform X;
            const int rule = merge_xform(a, (int32_t)a[12], (float)a[13], a[14], &X);
            if ((rule == MERGE_ARG_OK) != (merge_arg_text(rule) == nullptr)) return 3;
            print_xform(rule, X);
        } else if (line[0] == 'C') {
            double a[6];
            if (!doubles(&p, a, 6)) return 2;
            const int rule = merge_compat(a[0], a[1], a[2], a[3], (int)a[4], (int)a[5]);
            if ((rule == MERGE_COMPAT_OK) != (merge_compat_text(rule) == nullptr)) return 3;
            std::printf("%d\n", rule);
        } else if (line[0] == 'B') {
            double a[17];
            if (!doubles(&p, a, 17)) return 2;
            MergeXform X;
            const int mode = (int)a[13];
            if (merge_xform(a, mode, 0.0f, a[12], &X) != MERGE_ARG_OK) return 4;
            const int32_t B[3] = {(int32_t)a[14], (int32_t)a[15], (int32_t)a[16]};
            MergeBox bx;
            merge_brick_box(X, B, mode, &bx);
            std::printf("%" PRId32 " %" PRId32 " %" PRId32 " %" PRId32 " %" PRId32 " %" PRId32
                        " %a %" PRIu64 "\n",
                        bx.lo[0], bx.lo[1], bx.lo[2], bx.hi[0], bx.hi[1], bx.hi[2], bx.pad,
                        merge_box_pairs(bx));
        } else if (line[0] == 'S') {
            unsigned long long pairs;
            if (std::sscanf(p, "%llu", &pairs) != 1) return 2;
            std::printf("%" PRIu64 " %" PRIu64 "\n", merge_set_slots(pairs),
                        merge_scratch_bytes(pairs));
        } else {
            return 2;
        }
        n_q++;
    }
    std::printf("ok %llu\n", n_q);
    return 0;
}
