// The fault hook of the tests (hip_guard.h): which guarded HIP call fails.  A translation unit of its own, so that a
// program with another policy (tools/sanitize_viso.cpp: every n-th call of any kind) links its own fi_armed / fi_hit.
#include "hip_guard.h"

#include <stdlib.h>
#include <string.h>

#include <atomic>

namespace svh {

namespace {
std::atomic<int> g_fi_kind{-1};          // -1: nothing armed
std::atomic<int64_t> g_fi_first{0}, g_fi_count{1};
std::atomic<int64_t> g_fi_seen[FI_KINDS];
bool fi_parse(const char* spec) {
    static const char* names[FI_KINDS] = {"malloc", "launch", "copy", "wait"};
    g_fi_kind.store(-1);
    if (!spec || !*spec) return true;
    const char* colon = strchr(spec, ':');
    if (!colon) return false;
    int kind = -1;
    for (int k = 0; k < FI_KINDS; k++)
        if (strlen(names[k]) == (size_t)(colon - spec) && !strncmp(spec, names[k], colon - spec)) kind = k;
    if (kind < 0) return false;
    char* end = nullptr;
    const long long n = strtoll(colon + 1, &end, 10);
    long long cnt = 1;
    if (end && *end == ':') cnt = strtoll(end + 1, nullptr, 10);
    if (n < 1 || cnt < 0) return false;
    for (auto& c : g_fi_seen) c.store(0);
    g_fi_first.store(n);
    g_fi_count.store(cnt);
    g_fi_kind.store(kind);
    return true;
}
}   // namespace
bool fi_armed() { return g_fi_kind.load(std::memory_order_relaxed) >= 0; }
bool fi_hit(FiKind kind) {
    if (g_fi_kind.load(std::memory_order_relaxed) != (int)kind) return false;
    const int64_t i = g_fi_seen[kind].fetch_add(1) + 1, first = g_fi_first.load(), cnt = g_fi_count.load();
    return i >= first && (cnt == 0 || i < first + cnt);
}

}   // namespace svh

extern "C" int32_t svh_test_fail_at(const char* spec) {
    return svh::fi_parse(spec) ? SVH_OK : svh::fail(SVH_ERR_BAD_ARG, "bad fault specification");
}
