// The host arithmetic of the 2:1 coarsening (noetic-slam_amd/csrc/coarsen_plan.h) on the CPU:
// answers the queries on stdin, one per line, for tests/test_coarsen_plan.py to compare with its
// Python restatement over a grid:
//   A <side> <has_lo> <has_hi> <min_children> <min_weight %a|nan>  -> "<rule> <text|->"
//   C <vs_dst> <vs_src> <tau_dst> <tau_src> <sem_dst> <sem_src>    -> "<rule> <text|->"  (doubles, %a)
//   P <b>                                                         -> "<parent>"
//   S <has_box> <side> <lo x3> <hi x3> <b x3>                      -> "<selected 0|1>"
//   L <lane>                                     -> "<child brick> <child base> <offsets k = 0..7>"
//   Z <src_bricks>                                                -> "<set slots> <scratch bytes>"
// and prints "ok <queries>" at the end.  Built plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../noetic-slam_amd/csrc/coarsen_plan.h"

using namespace tsdf;

static void rule_line(int rule, const char* text) {
    std::printf("%d %s\n", rule, text ? text : "-");
}

int main() {
    char line[512];
    unsigned long long n_q = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == 'A') {
            int side, has_lo, has_hi;
            long long mc;
            char w[64];
            if (std::sscanf(line + 1, "%d %d %d %lld %63s", &side, &has_lo, &has_hi, &mc, w) != 5)
                return 2;
            const float mw = std::strcmp(w, "nan") == 0 ? NAN : (float)std::strtod(w, nullptr);
            const int r = coarsen_args(side, has_lo != 0, has_hi != 0, (uint32_t)mc, mw);
            rule_line(r, coarsen_arg_text(r));
        } else if (line[0] == 'C') {
            double a, b, c, d;
            int sa, sb;
            if (std::sscanf(line + 1, "%la %la %la %la %d %d", &a, &b, &c, &d, &sa, &sb) != 6)
                return 2;
            const int r = coarsen_compat(a, b, c, d, sa, sb);
            rule_line(r, coarsen_compat_text(r));
        } else if (line[0] == 'P') {
            int b;
            if (std::sscanf(line + 1, "%d", &b) != 1) return 2;
            std::printf("%d\n", coarsen_parent(b));
        } else if (line[0] == 'S') {
            CoarsenSel s{};
            int b[3];
            if (std::sscanf(line + 1, "%d %d %d %d %d %d %d %d %d %d %d", &s.has_box, &s.side,
                            &s.lo[0], &s.lo[1], &s.lo[2], &s.hi[0], &s.hi[1], &s.hi[2], &b[0],
                            &b[1], &b[2]) != 11)
                return 2;
            std::printf("%d\n", coarsen_selected(s, b[0], b[1], b[2]) ? 1 : 0);
        } else if (line[0] == 'L') {
            int l;
            if (std::sscanf(line + 1, "%d", &l) != 1 || l < 0 || l >= 512) return 2;
            std::printf("%d %d", coarsen_child_brick(l), coarsen_child_base(l));
            for (int k = 0; k < 8; k++) std::printf(" %d", coarsen_child_offset(k));
            std::printf("\n");
        } else if (line[0] == 'Z') {
            unsigned long long n;
            if (std::sscanf(line + 1, "%llu", &n) != 1) return 2;
            std::printf("%" PRIu64 " %" PRIu64 "\n", coarsen_set_slots(n), coarsen_scratch_bytes(n));
        } else {
            return 2;
        }
        n_q++;
    }
    std::printf("ok %llu\n", n_q);
    return 0;
}
