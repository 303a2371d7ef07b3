// Shared host-side helpers for libssd_hip.so (gfx950 only; no portability shims).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/ssd_hip.h"

namespace ssd {

void set_error(const char* fmt, ...);

#define SSD_CHECK_ARG(cond, ...)            \
    do {                                    \
        if (!(cond)) {                      \
            ssd::set_error(__VA_ARGS__);    \
            return SSD_E_INVALID;           \
        }                                   \
    } while (0)

#define SSD_UNSUPPORTED_IF(cond, ...)       \
    do {                                    \
        if (cond) {                         \
            ssd::set_error(__VA_ARGS__);    \
            return SSD_E_UNSUPPORTED;       \
        }                                   \
    } while (0)

#define SSD_HIP(call)                                                              \
    do {                                                                           \
        hipError_t e__ = (call);                                                   \
        if (e__ != hipSuccess) {                                                   \
            ssd::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                           __FILE__, __LINE__);                                    \
            return SSD_E_HIP;                                                      \
        }                                                                          \
    } while (0)

#define SSD_LAUNCH_CHECK()                                                        \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            ssd::set_error("kernel launch failed: %s (%s:%d)",                    \
                           hipGetErrorString(e__), __FILE__, __LINE__);           \
            return SSD_E_HIP;                                                     \
        }                                                                         \
    } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// the image I/O paths (preprocessing, Lanczos resize, drawing, JPEG): the largest height / width they take, so that a
// pixel's byte offset H * W * 3 stays below 2^31
static const int kMaxImageSide = 16384;
static inline bool image_side_ok(const int v) { return v >= 1 && v <= kMaxImageSide; }

// One image's region [offset, offset + length) of a buffer of `limit` bytes, as the ragged entry points require it:
// not negative, a multiple of `align` (a power of two; 1: any), inside the buffer and -- with `end`, the running end of
// the regions before it, which then moves to this region's end -- not before the previous image's region ends.
static inline bool region_ok(const long long offset, const size_t length, const size_t limit, const size_t align,
                             size_t* end = nullptr) {
    if (offset < 0 || ((size_t)offset & (align - 1)) != 0 || (end && (size_t)offset < *end) || (size_t)offset + length > limit)
        return false;
    if (end) *end = (size_t)offset + length;
    return true;
}

}  // namespace ssd
