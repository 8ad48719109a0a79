// frad_platform_gfx950.hpp -- the product's side of the seam: every primitive of frad_platform.hpp (which holds the
// contracts and is the only file that includes this one) as gfx950 builtins and instructions.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#define FRAD_DYN_SMEM(name) extern __shared__ __attribute__((aligned(16))) unsigned char name[]
#define FRAD_GPTR(T, p) ((__attribute__((address_space(1))) T*)(p))
#define FRAD_GCPTR(T, p) ((const __attribute__((address_space(1))) T*)(p))
#define FRAD_OPAQUE(x) asm volatile("" : "+v"(x))
#define FRAD_PIN(x) asm volatile("" : "+v"(x))
#define FRAD_CLOCK() __builtin_amdgcn_s_memtime()
#define FRAD_ASM_COMMENT(text) asm volatile("; " text)
#define FRAD_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define FRAD_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define FRAD_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" :: "i"(n) : "memory")
#define FRAD_LDS_ADD(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define FRAD_LDS_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define FRAD_NAP(n) __builtin_amdgcn_s_sleep(n)
#define FRAD_NT_LOAD(p) __builtin_nontemporal_load(p)
#define FRAD_NT_STORE(v, p) __builtin_nontemporal_store((v), (p))

namespace frad {

// ---- lane movement and reductions: no step goes through the LDS crossbar (a ds_bpermute pair per step otherwise) ----
template <int CTRL> __device__ __forceinline__ u64 dpp_move_u64(u64 v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, false);
    return (u64)(uint32_t)lo | ((u64)(uint32_t)hi << 32);
}
__device__ __forceinline__ u64 read_lane_u64(u64 v, int lane) {      // through SGPRs
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return (u64)lo | ((u64)hi << 32);
}
// (a statement macro, not a function: the compiler simplifies a function of its own before it inlines it, and the 64-bit
// integer sum of the Golomb coder then comes out as other instructions than the ones it was measured with)
#define FRAD_ROWS16_ALLREDUCE_U64(v, op) { \
    v = op(v, ::frad::dpp_move_u64<0xB1>(v));                /* quad_perm [1,0,3,2] */ \
    v = op(v, ::frad::dpp_move_u64<0x4E>(v));                /* quad_perm [2,3,0,1] */ \
    v = op(v, ::frad::dpp_move_u64<0x141>(v));               /* row_half_mirror */ \
    v = op(v, ::frad::dpp_move_u64<0x140>(v));               /* row_mirror */ \
}
__device__ __forceinline__ u64 wave_row_u64(u64 v, int row) { return read_lane_u64(v, 16 * row); }
__device__ __forceinline__ int wave_read_lane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ int wave_uniform_int(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ bool wave_any(bool b) { return __builtin_amdgcn_ballot_w64(b) != 0; }

// ---- bits ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bfe_u32(uint32_t word, int shift, int width) {
    return __builtin_amdgcn_ubfe(word, (unsigned)shift, (unsigned)width);
}
__device__ __forceinline__ int bfe_i32(uint32_t word, int shift, int width) {
    return __builtin_amdgcn_sbfe((int)word, (unsigned)shift, (unsigned)width);
}
__device__ __forceinline__ uint32_t wave_perm(uint32_t v, uint32_t sel) { return __builtin_amdgcn_perm(v, 0u, sel); }

// ---- arithmetic --------------------------------------------------------------------------------------------------------
// (fmax(fm, fabs(v)) costs two instructions: the compiler canonicalises the operand first)
__device__ __forceinline__ void absmax_acc(double& fm, double v) {
    asm("v_max_f64 %0, %1, |%2|" : "=v"(fm) : "v"(fm), "v"(v));
}
// (the compiler's tied v_fmac would keep the result inside the 128-bit load tuple that delivered a and b, i.e. four
// registers alive for a two-register value)
__device__ __forceinline__ double fma_free(double s, double b, double a) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(s), "v"(b), "v"(a));
    return r;
}
// class mask: bit 0 signalling NaN, 1 quiet NaN, 2 -Inf, 9 +Inf
__device__ __forceinline__ bool nonfinite_f32(float f) { return __builtin_amdgcn_classf(f, 0x207); }

// ---- memory ------------------------------------------------------------------------------------------------------------
template <int AUX> __device__ __forceinline__ void lds_dma16(const unsigned char* src, unsigned char* lds) {
    __builtin_amdgcn_global_load_lds(FRAD_GCPTR(void, src), (__attribute__((address_space(3))) void*)(lds), 16, 0, AUX);
}

// ---- approximate float32 instructions (not bit-equal to libm: see the contract) ------------------------------------------
__device__ __forceinline__ float p1w_sqrtf(float v) { return __builtin_amdgcn_sqrtf(v); }
__device__ __forceinline__ float k7_log2f(float v) { return __builtin_amdgcn_logf(v); }
__device__ __forceinline__ float k7_exp2f(float v) { return __builtin_amdgcn_exp2f(v); }
__device__ __forceinline__ float k7_rcpf(float v) { return __builtin_amdgcn_rcpf(v); }

}  // namespace frad
