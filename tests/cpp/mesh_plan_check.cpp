// The host planning of the indexed mesh (noetic-slam_amd/csrc/mesh_plan.h) on the CPU: answers the
// queries on stdin, one per line, for tests/test_mesh_plan.py to compare with its Python
// restatement:
//   B <has box> <lo x3> <hi x3>            (int64)
//        -> "<rule> <empty> <lo x3> <hi x3>" of mesh_box_check
//   L <lo x3> <hi x3> <n> <brick x y z> x n   (a clamped box, int32; brick coordinates)
//        -> "<examined> <listed> <brick x y z> x listed" of mesh_list_bricks over the sorted keys
//   P <n> <tcnt vcnt> x n
//        -> "<n_tri> <n_vert> <toff vbase> x n" of mesh_prefix
// and prints "ok <queries>" at the end.  Built plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../noetic-slam_amd/csrc/mesh_plan.h"

using namespace tsdf;

int main() {
    std::string line;
    unsigned long long n_q = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char what = 0;
        in >> what;
        if (what == 'B') {
            int has = 0;
            int64_t lo[3], hi[3];
            in >> has >> lo[0] >> lo[1] >> lo[2] >> hi[0] >> hi[1] >> hi[2];
            if (!in) return 2;
            MeshBox B;
            bool empty = false;
            const int rule = mesh_box_check((has & 1) ? lo : nullptr, (has & 2) ? hi : nullptr, &B,
                                            &empty);
            if ((rule == MESH_ARG_OK) != (mesh_arg_text(rule)[0] == 0)) return 3;
            if (rule != MESH_ARG_OK) {
                std::printf("%d\n", rule);
            } else {
                std::printf("%d %d %d %d %d %d %d %d\n", rule, (int)empty, B.lo[0], B.lo[1], B.lo[2],
                            B.hi[0], B.hi[1], B.hi[2]);
            }
        } else if (what == 'L') {
            MeshBox B;
            uint64_t n = 0;
            in >> B.lo[0] >> B.lo[1] >> B.lo[2] >> B.hi[0] >> B.hi[1] >> B.hi[2] >> n;
            if (!in) return 2;
            std::vector<uint64_t> keys(n), listed;
            for (uint64_t i = 0; i < n; i++) {
                int32_t b[3];
                in >> b[0] >> b[1] >> b[2];
                if (!in || !brick_coord_ok(b[0]) || !brick_coord_ok(b[1]) || !brick_coord_ok(b[2]))
                    return 2;
                keys[i] = brick_key_pack(b[0], b[1], b[2]);
            }
            std::sort(keys.begin(), keys.end(), brick_key_less_zyx);
            const uint64_t examined = mesh_list_bricks(keys, B, &listed);
            std::printf("%" PRIu64 " %zu", examined, listed.size());
            for (uint64_t k : listed)
                std::printf(" %d %d %d", brick_key_coord(k, 0), brick_key_coord(k, 1),
                            brick_key_coord(k, 2));
            std::printf("\n");
        } else if (what == 'P') {
            uint64_t n = 0;
            in >> n;
            if (!in) return 2;
            std::vector<uint32_t> t(n), v(n), vbase(n);
            std::vector<uint64_t> toff(n);
            for (uint64_t i = 0; i < n; i++) in >> t[i] >> v[i];
            if (!in) return 2;
            uint64_t n_tri = 0, n_vert = 0;
            mesh_prefix(t.data(), v.data(), n, toff.data(), vbase.data(), &n_tri, &n_vert);
            std::printf("%" PRIu64 " %" PRIu64, n_tri, n_vert);
            for (uint64_t i = 0; i < n; i++) std::printf(" %" PRIu64 " %" PRIu32, toff[i], vbase[i]);
            std::printf("\n");
        } else {
            return 2;
        }
        n_q++;
    }
    std::printf("ok %llu\n", n_q);
    return 0;
}
