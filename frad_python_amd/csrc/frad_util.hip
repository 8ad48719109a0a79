// frad_util.hip -- measurement aid: a plain device-to-device copy with the access shape of the transform kernels
// (16 bytes per lane, fully coalesced, grid-stride), so that "achievable HBM bandwidth" in bench.py / DESIGN.md is
// measured with the same instruction mix as the product instead of borrowed from a library memcpy.
#include "frad_launch.hpp"
#include "../../include/frad_hip.h"

namespace frad {

__global__ void __launch_bounds__(256) k_bench_copy(const v4u* __restrict__ src, v4u* __restrict__ dst, long long n16) {
    // one 16 KiB tile per block and step: four 16-byte loads in flight per lane, every wave instruction 1 KiB contiguous
    const long long tiles = (n16 + 1023) / 1024;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long i = t * 1024 + threadIdx.x;
        if (i + 768 < n16) {
            const v4u a = FRAD_NT_LOAD(FRAD_GCPTR(v4u, src) + i), b = FRAD_NT_LOAD(FRAD_GCPTR(v4u, src) + i + 256),
                      c = FRAD_NT_LOAD(FRAD_GCPTR(v4u, src) + i + 512), d = FRAD_NT_LOAD(FRAD_GCPTR(v4u, src) + i + 768);
            FRAD_NT_STORE(a, FRAD_GPTR(v4u, dst) + i); FRAD_NT_STORE(b, FRAD_GPTR(v4u, dst) + i + 256);
            FRAD_NT_STORE(c, FRAD_GPTR(v4u, dst) + i + 512); FRAD_NT_STORE(d, FRAD_GPTR(v4u, dst) + i + 768);
        } else {
            for (long long j = i; j < n16 && j < (t + 1) * 1024; j += 256) FRAD_GPTR(v4u, dst)[j] = FRAD_GCPTR(v4u, src)[j];
        }
    }
}

// ---- parity test of the seam (frad_platform.hpp): every exact primitive on caller-supplied lane inputs ----------------------
// One block of 128 threads = two waves per launch, one kernel per case group; tests/test_lane_prims.py holds the NumPy
// model and runs the same cases on the emulator build and on the device.  All arrays are [rows][128], row-major.
constexpr int kLpThreads = 128;
// in: u64 a[128] | double d[128].  out u64 [7][128]: all-reduce max(a), or(a), sum(d); half-wave max(a) lo, hi; half-wave sum(d) lo, hi
__global__ void __launch_bounds__(kLpThreads) k_lp_reduce(const u64* in, u64* out) {
    const int t = threadIdx.x;
    const u64 a = in[t];
    const double d = u2d(in[kLpThreads + t]);
    out[0 * kLpThreads + t] = wave_max_u64(a);
    out[1 * kLpThreads + t] = wave_allreduce_u64(a, [](u64 x, u64 y) { return x | y; });
    out[2 * kLpThreads + t] = wave_allreduce_u64(d2u(d), [](u64 x, u64 y) { return d2u(u2d(x) + u2d(y)); });
    u64 lo, hi;
    half_wave_max_u64(a, lo, hi);
    out[3 * kLpThreads + t] = lo; out[4 * kLpThreads + t] = hi;
    double sl, sh;
    half_wave_sum_f64(d, sl, sh);
    out[5 * kLpThreads + t] = d2u(sl); out[6 * kLpThreads + t] = d2u(sh);
}
// in: int v[128] | int src[2][4] (per wave) | int pred[3][128].  out int [8][128]: v of lane src[wave][0 .. 3]; v of the first
// lane; any(pred[0 .. 2])
__global__ void __launch_bounds__(kLpThreads) k_lp_uniform(const int* in, int* out) {
    const int t = threadIdx.x, w = wave_uniform_int(t >> 6);
    const int v = in[t];
    const int* src = in + kLpThreads + 4 * w;
    const int* pred = in + kLpThreads + 8;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k * kLpThreads + t] = wave_read_lane(v, wave_uniform_int(src[k]));
    out[4 * kLpThreads + t] = wave_uniform_int(v);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(5 + k) * kLpThreads + t] = wave_any(pred[k * kLpThreads + t] != 0) ? 1 : 0;
}
// in: uint32 word[128].  out int [16][128], row 8 sg + 4 wi + si: sg = 0 unsigned, 1 signed; width 8 << wi; shift 8 si
__global__ void __launch_bounds__(kLpThreads) k_lp_bfe(const uint32_t* in, int* out) {
    const int t = threadIdx.x;
    const uint32_t word = in[t];
#pragma unroll
    for (int wi = 0; wi < 2; ++wi)
#pragma unroll
        for (int si = 0; si < 4; ++si) {
            out[(4 * wi + si) * kLpThreads + t] = (int)bfe_u32(word, 8 * si, 8 << wi);
            out[(8 + 4 * wi + si) * kLpThreads + t] = bfe_i32(word, 8 * si, 8 << wi);
        }
}
// in: uint32 v[128] | uint32 sel[n].  out uint32 [n][128]
__global__ void __launch_bounds__(kLpThreads) k_lp_perm(const uint32_t* in, uint32_t* out, int n) {
    const int t = threadIdx.x;
    const uint32_t v = in[t];
    for (int k = 0; k < n; ++k) out[k * kLpThreads + t] = wave_perm(v, in[kLpThreads + k]);
}
// in: double fm[n] | v[n] | s[n] | b[n] | a[n] | float f[n] (n a multiple of 128).  out: u64 absmax[n] | u64 fma[n] | uint32 nonfinite[n]
__global__ void __launch_bounds__(kLpThreads) k_lp_arith(const double* in, u64* out, int n) {
    const float* f = reinterpret_cast<const float*>(in + 5 * (long long)n);
    uint32_t* nf = reinterpret_cast<uint32_t*>(out + 2 * (long long)n);
    for (int i = threadIdx.x; i < n; i += kLpThreads) {
        double fm = in[i];
        absmax_acc(fm, in[n + i]);
        out[i] = d2u(fm);
        out[n + i] = d2u(fma_free(in[2 * n + i], in[3 * n + i], in[4 * n + i]));
        nf[i] = nonfinite_f32(f[i]) ? 1u : 0u;
    }
}
// in: v4u dma_src[128] | v4u nt_src[128].  out v4u [3][128]: the wave's 1 KiB LDS image read back at the lane's own slot and at the
// mirrored one (slot 63 - lane: another lane's bytes), and nt_src through a nontemporal load and store
__global__ void __launch_bounds__(kLpThreads) k_lp_memory(const v4u* in, v4u* out) {
    FRAD_DYN_SMEM(smem);
    const int t = threadIdx.x, lane = t & 63, w = wave_uniform_int(t >> 6);
    unsigned char* wbuf = smem + 1024 * w;
    lds_dma16<2>(reinterpret_cast<const unsigned char*>(in + t), wbuf);
    FRAD_VMCNT(0);
    team_sync<64>();
    out[t] = *reinterpret_cast<const v4u*>(wbuf + 16 * lane);
    out[kLpThreads + t] = *reinterpret_cast<const v4u*>(wbuf + 16 * (63 - lane));
    FRAD_NT_STORE(FRAD_NT_LOAD(FRAD_GCPTR(v4u, in) + kLpThreads + t), FRAD_GPTR(v4u, out) + 2 * kLpThreads + t);
}

}  // namespace frad

// Not part of the C-ABI (not declared in frad_hip.h): the seam's parity test.  `group` 0 .. 5 selects the kernel above, `n` is the
// row count of groups 3 (selectors) and 4 (values, a multiple of 128) and ignored otherwise.
extern "C" int frad_debug_lane_prims(int group, const void* in, void* out, int64_t n, void* stream) {
    using namespace frad;
    if (!in || !out || !aligned16(in) || !aligned16(out)) return FRAD_E_INVALID;
    const dim3 one(1), th(kLpThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (group) {
        case 0: hipLaunchKernelGGL(k_lp_reduce, one, th, 0, s, static_cast<const u64*>(in), static_cast<u64*>(out)); break;
        case 1: hipLaunchKernelGGL(k_lp_uniform, one, th, 0, s, static_cast<const int*>(in), static_cast<int*>(out)); break;
        case 2: hipLaunchKernelGGL(k_lp_bfe, one, th, 0, s, static_cast<const uint32_t*>(in), static_cast<int*>(out)); break;
        case 3:
            if (n < 1 || n > 64) return FRAD_E_INVALID;
            hipLaunchKernelGGL(k_lp_perm, one, th, 0, s, static_cast<const uint32_t*>(in), static_cast<uint32_t*>(out), (int)n);
            break;
        case 4:
            if (n < kLpThreads || n > (1 << 20) || n % kLpThreads) return FRAD_E_INVALID;
            hipLaunchKernelGGL(k_lp_arith, one, th, 0, s, static_cast<const double*>(in), static_cast<u64*>(out), (int)n);
            break;
        case 5: hipLaunchKernelGGL(k_lp_memory, one, th, 2 * 1024, s, static_cast<const v4u*>(in), static_cast<v4u*>(out)); break;
        default: return FRAD_E_INVALID;
    }
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

extern "C" int frad_bench_copy(const void* src, void* dst, int64_t nbytes, void* stream) {
    if (nbytes < 0 || (nbytes & 15) || !frad::aligned16(src) || !frad::aligned16(dst)) return FRAD_E_INVALID;
    if (nbytes == 0) return FRAD_OK;
    if (!src || !dst) return FRAD_E_INVALID;
    const long long n16 = nbytes / 16;
    long long blocks = (n16 + 1023) / 1024;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(frad::k_bench_copy, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const frad::v4u*>(src), static_cast<frad::v4u*>(dst), n16);
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}
