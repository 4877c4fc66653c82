// The one place where a host engine's error is recorded and reported (hip_guard.h): the text behind svh_last_error(),
// and the outcome of a failed HIP call.  (The fault hook of the tests is svh_fault_hook.cpp.)
#include "hip_guard.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>

namespace svh {

static thread_local std::string t_error;

int fail(int code, const std::string& msg) {
    t_error = msg;
    return code;
}
void report_hip_failure(const char* entry) { fprintf(stderr, "svhip: %s: %s\n", entry, t_error.c_str()); }
int hip_failed(const char* entry, const char* expr_text, bool injected, hipError_t e) {
    const int rc = fail(SVH_ERR_HIP, std::string(expr_text) + ": " +
                                         (injected ? "injected failure (SVH_TEST_FAIL_AT)" : hipGetErrorString(e)));
    if (entry) report_hip_failure(entry);
    return rc;
}
double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

}   // namespace svh

extern "C" {
const char* svh_last_error(void) { return svh::t_error.c_str(); }
}
