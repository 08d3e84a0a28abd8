// kv_require.h -- how a host function refuses: the message goes to kv_set_error, the KV_* code is the function's result.  No HIP
// in it: the host rules kept in plain headers (kv_seq_jobs.h ...) refuse with it, and a test harness brings its own kv_set_error.
#pragma once

void kv_set_error(const char *fmt, ...);

#define KV_REQUIRE(cond, code, ...)                                                         \
    do {                                                                                    \
        if (!(cond)) { kv_set_error(__VA_ARGS__); return (code); }                          \
    } while (0)

// a step of a host function that returns a KV_* code: anything but KV_OK is the caller's result as well
#define KV_STEP(call)                                                                       \
    do {                                                                                    \
        const int rc__ = (call);                                                            \
        if (rc__ != KV_OK) return rc__;                                                     \
    } while (0)
