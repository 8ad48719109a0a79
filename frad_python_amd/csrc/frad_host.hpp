// frad_host.hpp -- what the host side of every translation unit shares: the library's one HIP error slot and its check
// macro, stream-ordered scratch, and the argument checks of the C-ABI entry points.  No device code.
#pragma once
#include "frad_platform.hpp"
#include "../../include/frad_hip.h"
#include <cstddef>
#include <initializer_list>

namespace frad {

// this thread's last failed HIP call, whichever file made it: what frad_last_hip_error() returns (defined in frad_hip.hip)
int& last_hip_slot();

// record a failed HIP call and leave with FRAD_E_HIP
#define FRAD_HIPCHK(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { ::frad::last_hip_slot() = (int)e_; return FRAD_E_HIP; } } while (0)

// stream-ordered scratch, released on every path out
struct Scratch {
    hipStream_t s; void* p = nullptr;
    explicit Scratch(hipStream_t st) : s(st) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { if (p) (void)hipFreeAsync(p, s); }
    int alloc(size_t bytes) {                                  // FRAD_OK / FRAD_E_NOMEM (the HIP code is recorded as well)
        const hipError_t e = hipMallocAsync(&p, bytes, s);
        if (e == hipSuccess) return FRAD_OK;
        last_hip_slot() = (int)e; p = nullptr;
        return FRAD_E_NOMEM;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// storage depths of the lossless profiles (0 and 4)
inline bool valid_bits(int b) { return b == 12 || b == 16 || b == 24 || b == 32 || b == 48 || b == 64; }
// FRAD_PCM_*: kind << 3 | log2(bytes) << 1 | big-endian; no 1-byte floats, no big-endian bytes
inline bool valid_pcm_dtype(int d) {
    if (d < 0 || d > 23) return false;
    const int kind = d >> 3, lg = (d >> 1) & 3, be = d & 1;
    return !(kind == 2 && lg == 0) && !(lg == 0 && be);
}
// profile2.py:7 DEPTHS (not profile 1's table)
inline bool valid_p2_depth(int bits) {
    for (int b : {8, 10, 12, 14, 16, 20, 24}) if (b == bits) return true;
    return false;
}

}  // namespace frad
