// How every host translation unit looks at the result of a HIP call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdexcept>
#include <string>

namespace kzg {

// a failed HIP call; `code` lets a caller tell an exhausted HBM (retry with a smaller sub-batch) from a broken device
struct HipError : std::runtime_error {
    hipError_t code;
    HipError(hipError_t c, const std::string& what) : std::runtime_error(what), code(c) {}
    bool out_of_memory() const { return code == hipErrorOutOfMemory || code == hipErrorMemoryAllocation; }
};
#define HIPCK(x)                                                                                              \
    do {                                                                                                      \
        hipError_t e_ = (x);                                                                                  \
        if (e_ != hipSuccess)                                                                                 \
            throw HipError(e_, std::string("HIP error: ") + hipGetErrorString(e_) + " at " + __FILE__ + ":" + \
                                   std::to_string(__LINE__));                                                 \
    } while (0)
// Kernel launches report failures only through the thread's last-error slot: look at it before trusting anything that
// is read back after the synchronisation (a stale status word or result point must never pass for a fresh one).
#define SYNC_CHECKED(stream)                 \
    do {                                     \
        HIPCK(hipGetLastError());            \
        HIPCK(hipStreamSynchronize(stream)); \
        HIPCK(hipGetLastError());            \
    } while (0)

}  // namespace kzg
