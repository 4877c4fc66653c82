// CPU driver over stereo-vision_amd/csrc/queue_plan.h (no HIP): prints the queue plan for every line of its input.
//   input line:   least greatest cap workers requested        (cap "-" = GPU_MAX_HW_QUEUES unset; else its text)
//   output line:  plan streams_per_lane classes queues  then per lane parity  nstreams c0 c1 c2 sA sS sB pA pS pB
// (c*: class of stream k, -1 past nstreams; s*: stream of phase A, S, B; p*: priority value the phase's stream is
// created with).  tests/test_queue_plan.py builds and reads it.
#include <stdio.h>
#include <string.h>

#include "../../stereo-vision_amd/csrc/queue_plan.h"

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int least, greatest, workers, requested;
        char cap_text[64];
        if (sscanf(line, "%d %d %63s %d %d", &least, &greatest, cap_text, &workers, &requested) != 5) return 2;
        const int cap = svh::queue_cap_from_text(strcmp(cap_text, "-") ? cap_text : nullptr);
        const svh::QueuePlan q = svh::make_queue_plan(least, greatest, cap, workers, requested);
        printf("%d %d %d %d", q.plan, q.streams_per_lane, q.classes, q.queues);
        for (int parity = 0; parity < 2; parity++) {
            const svh::QueueLane& L = q.lane[parity];
            printf("  %d", L.nstreams);
            for (int k = 0; k < svh::QC_COUNT; k++) printf(" %d", k < L.nstreams ? L.cls[k] : -1);
            for (int ph = 0; ph < svh::QPH_COUNT; ph++) printf(" %d", L.phase_stream[ph]);
            for (int ph = 0; ph < svh::QPH_COUNT; ph++)
                printf(" %d", svh::queue_priority_of(L.cls[L.phase_stream[ph]], least, greatest));
        }
        printf("\n");
    }
    return 0;
}
