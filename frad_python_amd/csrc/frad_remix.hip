// frad_remix.hip -- the channel mix behind StreamIndex.decode(..., channels=K): frad_clips_remix.
//
//   k_clips_remix  a small float64 matrix [C_out][C_in] applied to every row of many ragged float64 spans whose channel count
//                  differs per clip, in one launch, with frad_clips_window_add's output side: the conversion to any PCM format,
//                  ragged or scattered spans, silence padding, 16-byte stores where the address allows.
//
// For one source row x[0 .. C_in) and output channel k the terms are the c, ascending, with M[k][c] != 0.0: the first sets
// acc = x[c] * M[k][c], every later one does acc = acc + x[c] * M[k][c] -- a rounded multiply, then a rounded add, never an fma
// (the unit is built with -ffp-contract=off on both sides, and the product is a statement of its own).  A row of M without a
// non-zero entry gives +0.0.  Skipping the zero weights is the definition: an identity or permutation row copies the source's
// bits (x * 1.0 is exact: -0.0, denormals, +-Inf), and no Inf * 0 is ever formed.
#include "frad_p1.hpp"
#include "frad_launch.hpp"
#include "../../include/frad_hip.h"

namespace frad {
namespace {

// (the few store helpers of frad_epilogue.hip this unit needs, restated)
template <int LGS> __device__ __forceinline__ u64 rm_swap_elem(u64 b) {
    if constexpr (LGS == 1) return bswap16((uint32_t)b);
    else if constexpr (LGS == 2) return bswap32((uint32_t)b);
    else if constexpr (LGS == 3) return bswap64(b);
    else return b;
}
template <int LGS> __device__ __forceinline__ void rm_store_elem(unsigned char* p, u64 b) {
    if constexpr (LGS == 0) *FRAD_GPTR(unsigned char, p) = (unsigned char)b;
    else if constexpr (LGS == 1) *FRAD_GPTR(unsigned short, p) = (unsigned short)b;
    else if constexpr (LGS == 2) *FRAD_GPTR(uint32_t, p) = (uint32_t)b;
    else *FRAD_GPTR(u64, p) = b;
}
template <int LGS> __device__ __forceinline__ v4u rm_pack16(const u64* b) {
    v4u q = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < (16 >> LGS); ++e) {
        if constexpr (LGS == 3) { q[2 * e] = (uint32_t)b[e]; q[2 * e + 1] = (uint32_t)(b[e] >> 32); }
        else if constexpr (LGS == 2) q[e] = (uint32_t)b[e];
        else if constexpr (LGS == 1) q[e >> 1] |= (uint32_t)b[e] << (16 * (e & 1));
        else q[e >> 2] |= (uint32_t)b[e] << (8 * (e & 3));
    }
    return q;
}

struct RmTables {                                              // the per-clip tables (device memory)
    const double* const* src_ptr; const int32_t* src_ch; const int64_t* mat_off;
    const int32_t* valid; const int64_t* dst_row; const int64_t* out_off;
};
struct RmCur {                                                 // the clip a lane is in: its tables' entries, read once per clip
    long long j, base, end, shift;
    const double* src; const double* mat;                      // the clip's rows, and its matrix [C_out][cin]
    int cin, valid;
};

constexpr int REMIX_K = 4;

// The launch is partitioned by out_off in units of C_out elements, as frad_clips_window_add's is: a block owns a tile of
// REMIX_K * 256 stores of 16 bytes, a lane every 256th of them, and finds its clip by a binary search over out_off only when a
// store has left the clip.  The elements of a store lie in one or more output rows (C_out is small): the lane walks those rows,
// reads each source row's cin values once -- two at a time where the address is 16-byte aligned -- and feeds every value to the
// elements of that row, whose accumulators, row numbers and channels sit in registers (the loops over a store's elements are
// unrolled, so every index into them is a constant).  The matrix is read through the caches: it is a few doubles per clip and
// every lane of a clip reads the same ones.
template <int KIND, int LGS>
__global__ void __launch_bounds__(256) k_clips_remix(RmTables t, const double* __restrict__ mats, long long n_clips, int C,
                                                     unsigned char* __restrict__ out, long long out_rows, int be, int raw_be) {
    constexpr int EPT = 16 >> LGS;
    long long last = t.out_off[n_clips];
    if (last > out_rows) last = out_rows;                      // never beyond what the caller sized
    const long long n = last * C, n0 = (long long)t.out_off[0] * C;
    const long long tile = 256LL * EPT * REMIX_K;
    auto enter = [&](RmCur& k, long long j) {
        k.j = j; k.base = t.out_off[j]; k.end = t.out_off[j + 1];
        k.src = t.src_ptr[j]; k.cin = t.src_ch[j]; k.mat = mats + t.mat_off[j]; k.valid = t.valid[j];
        k.shift = t.dst_row != nullptr ? (long long)t.dst_row[j] - k.base : 0;
    };
    for (long long t0 = (long long)blockIdx.x * tile; t0 < n; t0 += (long long)gridDim.x * tile) {
        RmCur k;
        k.j = -1; k.end = 0;
        for (int it = 0; it < REMIX_K; ++it) {
            const long long i0 = t0 + ((long long)it * 256 + threadIdx.x) * EPT;
            if (i0 >= n) break;
            long long s;
            if (n <= 0x7fffffffLL) s = (uint32_t)i0 / (uint32_t)C; else s = i0 / C;
            const int c0 = (int)(i0 - s * C);
            if (k.j < 0 || s >= k.end) {                       // the last clip that starts at or before sample-frame s
                long long lo = k.j < 0 ? 0 : k.j, hi = n_clips;
                while (hi - lo > 1) {
                    const long long mid = (lo + hi) >> 1;
                    if ((long long)t.out_off[mid] <= s) lo = mid; else hi = mid;
                }
                enter(k, lo);
            }
            // one 16-byte store: all of it inside the launch, at an aligned address, and -- where the spans are scattered -- inside
            // the span of the clip its first sample is in
            const int n_rows = (int)((uint32_t)(c0 + EPT - 1) / (uint32_t)C) + 1;
            const long long s_last = s + n_rows - 1;
            unsigned char* const at = out + ((i0 + k.shift * C) << LGS);
            const bool vec = i0 >= n0 && i0 + EPT <= n && (t.dst_row == nullptr || s_last < k.end) &&
                             (reinterpret_cast<uintptr_t>(at) & 15) == 0;
            int row_of[EPT], ch_of[EPT];                       // element e of the store: row s + row_of[e], channel ch_of[e]
            double acc[EPT];
            u64 b[EPT];
            {
                int c = c0, r = 0;
#pragma unroll
                for (int e = 0; e < EPT; ++e) {
                    row_of[e] = r; ch_of[e] = c; acc[e] = 0.0;
                    if (++c == C) { c = 0; ++r; }
                }
            }
            for (int rr = 0; rr < n_rows; ++rr) {
                const long long sr = s + rr;
                while (sr >= k.end && k.j + 1 < n_clips) enter(k, k.j + 1);
                const long long r = sr - k.base;
                if (r >= 0 && r < k.valid && sr < last) {      // (else: padding, or a row outside the launch -- 0.0)
                    const int cin = k.cin;
                    const double* const x = k.src + r * cin;
                    uint32_t started = 0;                      // bit e: element e has its first term
                    auto term = [&](double v, int ci) {
#pragma unroll
                        for (int e = 0; e < EPT; ++e) {
                            if (row_of[e] == rr) {
                                const double m = *FRAD_GCPTR(double, k.mat + (long long)ch_of[e] * cin + ci);
                                if (m != 0.0) {
                                    const double p = v * m;
                                    acc[e] = (started >> e & 1u) ? acc[e] + p : p;
                                    started |= 1u << e;
                                }
                            }
                        }
                    };
                    int ci = 0;
                    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) { term(*FRAD_GCPTR(double, x), 0); ci = 1; }
                    for (; ci + 1 < cin; ci += 2) {
                        const v2d v = *FRAD_GCPTR(v2d, x + ci);
                        term(v[0], ci);
                        term(v[1], ci + 1);
                    }
                    if (ci < cin) term(*FRAD_GCPTR(double, x + ci), ci);
                }
#pragma unroll
                for (int e = 0; e < EPT; ++e) {
                    if (row_of[e] == rr) {
                        b[e] = from_f64_bits<KIND, LGS>(acc[e], raw_be != 0 && be);
                        if (be) b[e] = rm_swap_elem<LGS>(b[e]);
                        if (!vec && i0 + e < n && i0 + e >= n0) rm_store_elem<LGS>(out + ((i0 + e + k.shift * C) << LGS), b[e]);
                    }
                }
            }
            if (vec) FRAD_NT_STORE(rm_pack16<LGS>(b), FRAD_GPTR(v4u, at));
        }
    }
}

}  // namespace
}  // namespace frad

using namespace frad;

extern "C" {

int frad_clips_remix(const double* const* src_ptr, const int32_t* src_ch, const double* mats, const int64_t* mat_off, int64_t n_clips,
                     int32_t C_out, const int32_t* valid, const int64_t* dst_row, int32_t out_dtype, uint32_t flags, void* out,
                     const int64_t* out_off, int64_t out_rows, void* stream) {
    if (!valid_pcm_dtype(out_dtype) || n_clips < 0 || out_rows < 0 || C_out < 1) return FRAD_E_INVALID;
    if (n_clips == 0 || out_rows == 0) return FRAD_OK;
    if (!src_ptr || !src_ch || !mats || !mat_off || !valid || !out_off || !out) return FRAD_E_INVALID;
    const int kind = out_dtype >> 3, lg = (out_dtype >> 1) & 3, be = out_dtype & 1, raw = (flags & FRAD_RAW_BE_INTS) ? 1 : 0;
    const long long total = (long long)out_rows * C_out, per_block = 256LL * (16 >> lg) * REMIX_K;
    long long blocks = (total + per_block - 1) / per_block;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* o = static_cast<unsigned char*>(out);
    const RmTables t{src_ptr, src_ch, mat_off, valid, dst_row, out_off};
#define GO(KD, L) hipLaunchKernelGGL((k_clips_remix<KD, L>), grid, blk, 0, s, t, mats, (long long)n_clips, (int)C_out, o, (long long)out_rows, be, raw)
    switch (kind * 4 + lg) {
        case 0: GO(0, 0); break; case 1: GO(0, 1); break; case 2: GO(0, 2); break; case 3: GO(0, 3); break;
        case 4: GO(1, 0); break; case 5: GO(1, 1); break; case 6: GO(1, 2); break; case 7: GO(1, 3); break;
        case 9: GO(2, 1); break; case 10: GO(2, 2); break; case 11: GO(2, 3); break;
        default: return FRAD_E_INVALID;
    }
#undef GO
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

}  // extern "C"
