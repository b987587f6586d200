// launch_plan_check -- drives plan_launch of volrend_amd/csrc/vr_launch_plan.cpp for tests/test_launch_plan.py.
// Plain host build: no HIP, no library.  One query per line of standard input, one answer per line:
//   <kind: colour|aov|weights|backward> <source: frames|list> <n_frames> <list_rays> <lookup_bytes> [knob=value ...]
//       -> "chunk_max super_block raygen_waves records_nt frame_group n_queues"
// The knobs start from a default-constructed Tuning (every rule on auto).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "vr_launch_plan.h"

static bool set_knob(Tuning& tn, const char* key, int v) {
    struct { const char* key; int Tuning::*field; } const knobs[] = {
        {"chunk_max", &Tuning::chunk_max},       {"super_block", &Tuning::super_block},
        {"raygen_waves", &Tuning::raygen_waves}, {"records_nt", &Tuning::records_nt},
        {"frame_group", &Tuning::frame_group},   {"xcd_queues", &Tuning::xcd_queues},
    };
    for (const auto& k : knobs)
        if (!strcmp(key, k.key)) return tn.*k.field = v, true;
    return false;
}

int main() {
    char line[512];
    while (fgets(line, sizeof(line), stdin)) {
        char kind_s[16], source_s[16];
        int n_frames, at = 0;
        int64_t list_rays;
        uint64_t lookup_bytes;
        if (sscanf(line, "%15s %15s %d %" SCNd64 " %" SCNu64 "%n", kind_s, source_s, &n_frames, &list_rays,
                   &lookup_bytes, &at) != 5)
            return 2;
        const char* const kinds[] = {"colour", "aov", "weights", "backward"};
        const LaunchKind kind_of[] = {LaunchKind::kColour, LaunchKind::kAov, LaunchKind::kWeights, LaunchKind::kBackward};
        int kind = 0;
        while (kind < 4 && strcmp(kind_s, kinds[kind])) ++kind;
        const bool list = !strcmp(source_s, "list");
        if (kind == 4 || (!list && strcmp(source_s, "frames"))) return 2;
        Tuning tn;
        for (char* tok = strtok(line + at, " \n"); tok; tok = strtok(nullptr, " \n")) {
            char* eq = strchr(tok, '=');
            if (!eq) return 2;
            *eq = 0;
            if (!set_knob(tn, tok, atoi(eq + 1))) return 2;
        }
        const LaunchPlan p = plan_launch(kind_of[kind], list ? RaySource::kList : RaySource::kFrames,
                                         n_frames, list_rays, tn, lookup_bytes);
        printf("%d %d %d %d %d %d\n", p.chunk_max, p.super_block, p.raygen_waves, p.records_nt, p.frame_group,
               p.n_queues);
    }
    return 0;
}
