// CPU driver over stereo-vision_amd/csrc/group_feed.h (no HIP): K threads draw the groups of one batch call, with
// random short sleeps between their draws, as the engine's workers do between their lanes' steps.
//   input line:   fixed workers ngroups seed          (fixed: 1 = fixed shares, 0 = on demand)
//   output line:  one "w:i0,i1,..." field per worker, in the order the worker drew them ("w:" alone: it drew none),
//                 then "end:" and the number of draws that returned -1
// tests/test_group_feed.py builds it (once more under ThreadSanitizer) and checks what the engine relies on.
#include <stdint.h>
#include <stdio.h>

#include <chrono>
#include <random>
#include <thread>
#include <vector>

#include "../../stereo-vision_amd/csrc/group_feed.h"

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int fixed, workers, ngroups;
        unsigned seed;
        if (sscanf(line, "%d %d %d %u", &fixed, &workers, &ngroups, &seed) != 4 || workers < 1 || workers > 64) return 2;
        svh::GroupFeed feed;
        std::vector<std::vector<int32_t>> got(workers);
        std::vector<int> ends(workers, 0);
        std::vector<std::thread> th;
        for (int w = 0; w < workers; w++)
            th.emplace_back([&, w]() {
                std::mt19937 rng(seed * 977u + (unsigned)w);
                svh::FeedCursor cur;
                // (two more draws after the first -1: an exhausted feed stays exhausted)
                for (int after = 0; after < 3;) {
                    const int32_t peek = svh::feed_peek(feed, cur, fixed != 0, w, workers, ngroups);
                    const int32_t gi = svh::feed_take(feed, cur, fixed != 0, w, workers, ngroups);
                    if (gi < 0) {
                        after++;
                        ends[w]++;
                    } else {
                        if (after) ends[w] = -1000;              // a group after the end
                        if (fixed && peek != gi) ends[w] = -2000;   // fixed shares: the peek is exact
                        got[w].push_back(gi);
                    }
                    if (ngroups <= 64 || rng() % 8 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 60));
                }
            });
        for (std::thread& t : th) t.join();
        int total_ends = 0;
        for (int w = 0; w < workers; w++) {
            printf("%d:", w);
            for (size_t i = 0; i < got[w].size(); i++) printf(i ? ",%d" : "%d", got[w][i]);
            printf(" ");
            total_ends += ends[w];
        }
        printf("end:%d\n", total_ends);
    }
    return 0;
}
