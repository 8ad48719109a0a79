// frad_platform_emu.hpp -- the emulator's side of the seam: the plain definition of every primitive of frad_platform.hpp
// (which holds the contracts and is the only file that includes this one, after tests/emu/hip_emu.hpp: the thread-per-lane
// interpreter, its HIP runtime shim and the macros it has always held -- FRAD_DYN_SMEM, FRAD_OPAQUE, FRAD_PIN, FRAD_GPTR,
// FRAD_GCPTR, FRAD_LDS_BARRIER).  Test build only; never part of libfrad_hip.so.
#pragma once

#define FRAD_CLOCK() 0ull
#define FRAD_ASM_COMMENT(text) ((void)0)
#define FRAD_LGKM0() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define FRAD_VMCNT(n) ((void)0)
#define FRAD_LDS_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_SEQ_CST)
#define FRAD_LDS_LOAD(p) __atomic_load_n((p), __ATOMIC_SEQ_CST)
#define FRAD_NAP(n) std::this_thread::yield()
#define FRAD_ROWS16_ALLREDUCE_U64(v, op) { for (int off_ = 1; off_ < 16; off_ <<= 1) v = op(v, __shfl_xor(v, off_, 64)); }
#define FRAD_NT_LOAD(p) (*(p))
#define FRAD_NT_STORE(v, p) (*(p) = (v))

namespace frad {
inline u64 wave_row_u64(u64 v, int row) { return __shfl(v, 16 * row, 64); }
inline int wave_read_lane(int v, int src) { return (int)__shfl((unsigned long long)(unsigned)v, src, 64); }
inline int wave_uniform_int(int v) { return (int)__shfl((unsigned long long)(unsigned)v, 0, 64); }
inline bool wave_any(bool b) {
    unsigned long long v = b ? 1 : 0;
    for (int off = 1; off < 64; off <<= 1) v |= __shfl_xor(v, off, 64);
    return v != 0;
}
inline uint32_t bfe_u32(uint32_t word, int shift, int width) { return (word >> shift) & ((1u << width) - 1u); }
inline int bfe_i32(uint32_t word, int shift, int width) {
    const int w = width < 32 - shift ? width : 32 - shift;     // a field that would pass bit 31 ends there
    return (int)((word >> shift) << (32 - w)) >> (32 - w);
}
inline uint32_t wave_perm(uint32_t v, uint32_t sel) {
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) { const uint32_t s = (sel >> (8 * i)) & 0xffu; r |= (s >= 4 && s < 8 ? (v >> (8 * (s - 4))) & 0xffu : 0u) << (8 * i); }
    return r;
}
inline void absmax_acc(double& fm, double v) { fm = std::fmax(fm, std::fabs(v)); }
inline double fma_free(double s, double b, double a) { return std::fma(s, b, a); }
inline bool nonfinite_f32(float f) { return !std::isfinite(f); }
template <int AUX> inline void lds_dma16(const unsigned char* src, unsigned char* lds) {      // each lane copies its own 16 bytes
    *reinterpret_cast<v4u*>(lds + (emu::t_idx.x & 63) * 16) = *reinterpret_cast<const v4u*>(src);
}
// approximate on gfx950, libm here: not bit-equal (see the contract)
inline float p1w_sqrtf(float v) { return sqrtf(v); }
inline float k7_log2f(float v) { return log2f(v); }
inline float k7_exp2f(float v) { return exp2f(v); }
inline float k7_rcpf(float v) { return 1.0f / v; }
}  // namespace frad
