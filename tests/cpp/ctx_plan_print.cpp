// Prints the context's sizing plan (noetic-slam_amd/csrc/ctx_plan.h) for the parameter sets on the
// command line, one line per set, so that a test can hold real walks against the header's own
// numbers instead of a restatement of them (tests/bandref.py plan_of).  Each argument is
//   voxel_size,sdf_trunc,semantics,walk,space_carving,max_range,voxblox_method,depth_weight,
//   allow_clear,max_points,max_batch
// (doubles as strtod reads them, "inf" included; the enums as their TSDF_* integers), and gives
//   maxp spr nstep fused band_vox
// or "refused: <text>".  Links no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../noetic-slam_amd/csrc/ctx_plan.h"

using namespace tsdf;

// the device constants (tsdf_device.h), as literals, as tests/cpp/ctx_plan_check.cpp has them
static const PlanConsts kConsts{1024, 512, 512, 4, 1 << 23};

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        double f[11];
        char* s = argv[a];
        for (int k = 0; k < 11; k++) {
            char* end;
            f[k] = std::strtod(s, &end);
            if (end == s || (k < 10 ? *end != ',' : *end != '\0')) {
                std::fprintf(stderr, "bad parameter set: %s\n", argv[a]);
                return 2;
            }
            s = end + 1;
        }
        tsdf_params p;
        std::memset(&p, 0, sizeof p);
        p.voxel_size = f[0];
        p.sdf_trunc = f[1];
        p.semantics = (int32_t)f[2];
        p.walk = (int32_t)f[3];
        p.space_carving = (int32_t)f[4];
        p.max_range = f[5];
        p.voxblox_method = (int32_t)f[6];
        p.depth_weight = (int32_t)f[7];
        p.allow_clear = (int32_t)f[8];
        p.max_points = (uint64_t)f[9];
        p.max_batch = (uint32_t)f[10];
        p.weight_mode = TSDF_WEIGHT_CONSTANT;
        p.max_bricks = 1u << 14;
        p.brick_side = TSDF_BRICK_SIDE;
        p.sector_input = TSDF_SECTOR_INPUT_FANOUT;
        p.sector_rule = TSDF_SECTOR_RULE_INDEX;
        p.use_weight_dropoff = 1;
        p.max_weight = 10000.0f;
        if (!params_valid(p)) {
            std::printf("refused: invalid\n");
            continue;
        }
        const CtxPlan P = ctx_plan(p, kConsts);
        if (!P.refusal.empty()) {
            std::printf("refused: %s\n", P.refusal.c_str());
            continue;
        }
        std::printf("%u %u %d %d %d\n", P.maxp, P.spr, P.nstep, P.fused ? 1 : 0, P.band_vox);
    }
    return 0;
}
