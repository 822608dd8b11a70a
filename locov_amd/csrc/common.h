// Shared host-side helpers for liblocov_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/locov_hip.h"

namespace locov {

// thread-local error message returned by locov_last_error()
char *err_buf();
int set_error(int code, const char *fmt, ...);

inline hipStream_t as_stream(locov_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Checks the launch that was just enqueued (no synchronisation).
int check_launch(const char *what);

// Raises `kernel`'s dynamic LDS limit to `bytes`, once per device a launch is made on (the attribute belongs to the kernel's code
// object on ONE device).  per_device_state: the caller's `static std::atomic<int> [kMaxDevices]` for that kernel (0 = not asked yet,
// 1 = raised, -1 = refused).  LOCOV_OK, or LOCOV_ERR_LAUNCH after set_error -- with who == nullptr the error text is left alone (a
// caller for which a refusal is no error).  The state remembers the FIRST call's answer: a kernel is always raised to one constant.
constexpr int kMaxDevices = 64;
int raise_dynamic_lds(std::atomic<int> *per_device_state, const void *kernel, int bytes, const char *who);

constexpr int kWave = 64;

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace locov

#define LOCOV_REQUIRE(cond, ...)                                          \
    do {                                                                  \
        if (!(cond)) return locov::set_error(LOCOV_ERR_INVALID_ARG, __VA_ARGS__); \
    } while (0)
