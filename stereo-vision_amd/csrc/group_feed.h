// Group feed of the ELAS engine's batch entries: which group a worker of a batch call gets next.  Pure arithmetic over
// one atomic counter -- no HIP call, no environment access -- so that the rule can be checked on the CPU
// (tests/cxx/group_feed_check.cpp, tests/test_group_feed.py).  See DESIGN.md, "Group feed".
//
// A batch call cuts its pairs into `ngroups` groups and runs them on `workers` workers of two lanes each.
//   * fixed shares: worker w gets the groups w, w + workers, w + 2 workers, ...  Right while every worker is equally
//     fast; where lanes share hardware queues unevenly the fast workers end early and stand idle.
//   * on demand: a worker's first group is still group w (no worker can be left without one by a quicker neighbour's
//     prefetch), every later one is drawn from a counter of the call that starts at `workers`.
// Either way every index in [0, ngroups) is handed out exactly once, and a worker's indices ascend.  Statuses and
// outputs are addressed by the group index, so the order in which groups complete cannot show in a result.
#ifndef SVH_GROUP_FEED_H
#define SVH_GROUP_FEED_H

#include <stdint.h>

#include <atomic>

namespace svh {

// SVH_FEED, a bit set read once per batch call: each bit brings back one behaviour of the engine before the feed
// (A/B runs); 0 is the default, 7 all three.
enum {
    FEED_PARITY_AT_ACQUIRE = 1,   // a lane's parity is its position in the acquisition, not a property of the lane
    FEED_FIXED_SHARES = 2,        // groups in fixed round-robin shares
    FEED_ALTERNATE = 4,           // a worker refills its two lanes in strict alternation
    FEED_ALL = 7,
};
inline int feed_mode_from_text(const char* text) {
    if (!text || !*text) return 0;
    int v = 0;
    for (const char* c = text; *c >= '0' && *c <= '9' && v < 1000; c++) v = v * 10 + (*c - '0');
    return v & FEED_ALL;
}

// one per batch call
struct GroupFeed {
    std::atomic<int32_t> next{0};   // on demand: draws made beyond the workers' first groups
};
// one per worker of the call
struct FeedCursor {
    int32_t taken = 0;              // groups this worker was handed so far
};

// the index a draw of worker `w` would return if it were made now and nobody else drew first; -1: none left
inline int32_t feed_peek(const GroupFeed& f, const FeedCursor& c, bool fixed, int w, int workers, int32_t ngroups) {
    if (workers < 1 || w < 0 || w >= workers) return -1;
    int64_t gi;
    if (fixed || c.taken == 0) gi = (int64_t)w + (int64_t)c.taken * workers;
    else gi = (int64_t)workers + f.next.load(std::memory_order_relaxed);
    return gi < ngroups ? (int32_t)gi : -1;
}

// the next group of worker `w` (0 <= w < workers), or -1 when the call has none left for it
inline int32_t feed_take(GroupFeed& f, FeedCursor& c, bool fixed, int w, int workers, int32_t ngroups) {
    if (feed_peek(f, c, fixed, w, workers, ngroups) < 0) return -1;   // (also keeps the counter from running away)
    int64_t gi;
    if (fixed || c.taken == 0) gi = (int64_t)w + (int64_t)c.taken * workers;
    else gi = (int64_t)workers + f.next.fetch_add(1, std::memory_order_relaxed);
    if (gi >= ngroups) return -1;
    c.taken++;
    return (int32_t)gi;
}

}  // namespace svh
#endif
