// Host-only driver of conv_bb_form_cost (csrc/conv_bb.hip): prints, per "B H W cus" line of its arguments, the MFMAs per wave of the busiest
// workgroup in the tile form and in the walk form of the fused 64-channel block, and the form conv_bb_launch takes with no FID_BB_V set.
// Compiled against csrc/conv.h and linked to the built library by tests/test_bb_walk_cpu.py; no device is touched.
#include <cstdio>
#include <cstdlib>

#include "../scrfd_arcface_facerecognition_amd/csrc/conv.h"

int main(int argc, char **argv) {
    for (int i = 1; i + 3 < argc; i += 4) {
        long long tile = 0, walk = 0;
        fid::conv_bb_form_cost(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), &tile, &walk);
        printf("%lld %lld %s\n", tile, walk, walk < tile ? "walk" : "tile");
    }
    return 0;
}
