// frad_resample.hip -- the polyphase resampler behind StreamIndex.decode(..., srate=R): frad_clips_resample.
//
//   k_clips_resample  scipy.signal.resample_poly's arithmetic (zero extension, the Kaiser-windowed sinc the host computes) on many
//                     ragged float64 spans in one launch, with frad_clips_window_add's output side: the conversion to any PCM
//                     format, ragged or scattered spans, silence padding, 16-byte stores where the address allows.
//
// For a stream resampled by up / down with taps h[0 .. 2 * half], half = 10 * max(up, down):
//   y[n][c] = sum over i ascending of x[i][c] * h[n * down - i * up + half],   ceil((n * down - half) / up) <= i <= floor((n * down + half) / up)
// with i clipped to the rows the clip holds, as acc = fma(x, h, acc) from acc = 0.0.  Both code paths below (source rows staged
// in LDS, source rows read from global memory) run that one loop in that order, so a row's value does not depend on the window
// that asked for it, on the tile it fell into or on the output format.  n * down and i * up are 64-bit.
#include "frad_p1.hpp"
#include "frad_launch.hpp"
#include "../../include/frad_hip.h"

namespace frad {
namespace {

// (the few store helpers of frad_epilogue.hip this unit needs, restated)
template <int LGS> __device__ __forceinline__ u64 rs_swap_elem(u64 b) {
    if constexpr (LGS == 1) return bswap16((uint32_t)b);
    else if constexpr (LGS == 2) return bswap32((uint32_t)b);
    else if constexpr (LGS == 3) return bswap64(b);
    else return b;
}
template <int LGS> __device__ __forceinline__ void rs_store_elem(unsigned char* p, u64 b) {
    if constexpr (LGS == 0) *FRAD_GPTR(unsigned char, p) = (unsigned char)b;
    else if constexpr (LGS == 1) *FRAD_GPTR(unsigned short, p) = (unsigned short)b;
    else if constexpr (LGS == 2) *FRAD_GPTR(uint32_t, p) = (uint32_t)b;
    else *FRAD_GPTR(u64, p) = b;
}
template <int LGS> __device__ __forceinline__ v4u rs_pack16(const u64* b) {
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

struct RsTables {                                              // the per-clip tables (device memory)
    const int64_t* src_off; const int64_t* src_row0; const int32_t* src_rows;
    const int64_t* out_row0; const int32_t* valid; const int64_t* dst_row; const int64_t* out_off;
};
struct RsCur {                                                 // the clip a lane is in: its tables' entries, read once per clip
    long long j, base, end, soff, s0, n0, shift;               // s0: the span's first row on the stream's timeline; n0: out_row0
    int rows, valid;
};
struct RsRow {                                                 // one output row: its terms are source rows [lo, hi], the first tap is k0
    long long lo, hi, k0;
};

// the source rows output row n reads, clipped to the rows [s0, s0 + rows) the clip holds; lo > hi: none
__device__ __forceinline__ RsRow rs_row(long long n, int up, int down, int half, long long s0, int rows) {
    const long long centre = n * down;
    RsRow r;
    const long long num = centre - half;
    r.lo = num > 0 ? (num + up - 1) / up : 0;                  // ceil; rows before the stream's first are zero
    r.hi = (centre + half) / up;
    if (r.lo < s0) r.lo = s0;
    if (r.hi > s0 + rows - 1) r.hi = s0 + rows - 1;
    r.k0 = centre - r.lo * up + half;                          // 0 <= k0 - (i - lo) * up <= 2 * half for every lo <= i <= hi
    return r;
}

constexpr int RS_LDS_BYTES = 48 * 1024;                        // the staged source rows of one tile: three blocks per CU, no opt-in
constexpr int RS_K_MAX = 8;

// The launch is partitioned by out_off as frad_clips_window_add's is: a block owns a tile of K * 256 stores of 16 bytes, a lane
// every 256th of them, and finds its clip by a binary search over out_off only when a store has left the clip.  A tile that lies
// inside one clip -- the common case: a window is hundreds of rows -- first stages the source rows its output rows read in LDS
// (every staged row is then read about 2 * half / down times from there instead of from L2), when they fit; the host sizes K so
// that they do for the clips' ratio and channel count.  Every other tile reads the source rows from global memory.  The taps
// are read through L2 (the table of 44.1 kHz -> 16 kHz is 69 KiB and every block reads all of it).
template <int KIND, int LGS>
__global__ void __launch_bounds__(256) k_clips_resample(const double* __restrict__ src, RsTables t, long long n_clips, int C, int up, int down,
                                                        const double* __restrict__ taps, int half, unsigned char* __restrict__ out,
                                                        long long out_rows, int be, int raw_be, int K) {
    constexpr int EPT = 16 >> LGS;
    FRAD_DYN_SMEM(smem);
    double* const staged = reinterpret_cast<double*>(smem);
    long long last = t.out_off[n_clips];
    if (last > out_rows) last = out_rows;                      // never beyond what the caller sized
    const long long n = last * C, n0 = (long long)t.out_off[0] * C;
    const long long tile = 256LL * EPT * K;
    auto enter = [&](RsCur& k, long long j) {
        k.j = j; k.base = t.out_off[j]; k.end = t.out_off[j + 1];
        k.soff = t.src_off[j]; k.s0 = t.src_row0[j]; k.rows = t.src_rows[j]; k.n0 = t.out_row0[j]; k.valid = t.valid[j];
        k.shift = t.dst_row != nullptr ? (long long)t.dst_row[j] - k.base : 0;
    };
    auto find = [&](long long s, long long from) {             // the last clip that starts at or before sample-frame s
        long long lo = from, hi = n_clips;
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if ((long long)t.out_off[mid] <= s) lo = mid; else hi = mid;
        }
        return lo;
    };
    for (long long t0 = (long long)blockIdx.x * tile; t0 < n; t0 += (long long)gridDim.x * tile) {
        // ---- the same in every lane of the block: is the tile inside one clip, and do the source rows it reads fit in LDS?
        long long st_lo = 0, st_rows = 0;                      // the staged source rows [st_lo, st_lo + st_rows) of the timeline
        {
            const long long b0 = t0 > n0 ? t0 : n0, b1 = t0 + tile < n ? t0 + tile : n;
            if (b0 < b1) {
                const long long s_first = b0 / C, s_last = (b1 - 1) / C;
                RsCur k;
                enter(k, find(s_first, 0));
                if (s_last < k.end && k.rows > 0) {
                    const long long r_lo = s_first - k.base;
                    long long r_hi = s_last - k.base;
                    if (r_hi > k.valid - 1) r_hi = k.valid - 1;
                    if (r_lo <= r_hi) {
                        const long long lo = rs_row(k.n0 + r_lo, up, down, half, k.s0, k.rows).lo;
                        const long long hi = rs_row(k.n0 + r_hi, up, down, half, k.s0, k.rows).hi;
                        if (lo <= hi && (hi - lo + 1) * C <= RS_LDS_BYTES / 8) {
                            st_lo = lo; st_rows = hi - lo + 1;
                            const double* from = src + k.soff + (lo - k.s0) * C;
                            for (long long e = threadIdx.x; e < st_rows * C; e += 256) staged[e] = from[e];
                        }
                    }
                }
            }
        }
        if (st_rows) __syncthreads();
        RsCur k;
        k.j = -1; k.end = 0;
        for (int it = 0; it < K; ++it) {
            const long long i0 = t0 + ((long long)it * 256 + threadIdx.x) * EPT;
            if (i0 >= n) break;
            long long s;
            if (n <= 0x7fffffffLL) s = (uint32_t)i0 / (uint32_t)C; else s = i0 / C;
            int c = (int)(i0 - s * C);
            if (k.j < 0 || s >= k.end) enter(k, find(s, k.j < 0 ? 0 : k.j));
            // one 16-byte store: all of it inside the launch, at an aligned address, and -- where the spans are scattered -- inside
            // the span of the clip its first sample is in
            const long long s_last = s + (uint32_t)(c + EPT - 1) / (uint32_t)C;
            unsigned char* const at = out + ((i0 + k.shift * C) << LGS);
            const bool vec = i0 >= n0 && i0 + EPT <= n && (t.dst_row == nullptr || s_last < k.end) &&
                             (reinterpret_cast<uintptr_t>(at) & 15) == 0;
            RsRow row;
            row.lo = 0; row.hi = -1; row.k0 = 0;
            bool have = false, pad = false;
            u64 b[EPT];
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const bool live = i0 + e < n && i0 + e >= n0;
                double acc = 0.0;
                if (live) {
                    if (!have || c == 0) {
                        while (s >= k.end && k.j + 1 < n_clips) enter(k, k.j + 1);
                        const long long r = s - k.base;
                        pad = r >= k.valid;
                        if (!pad) row = rs_row(k.n0 + r, up, down, half, k.s0, k.rows);
                        have = true;
                    }
                    if (!pad && row.lo <= row.hi) {
                        const double* h = taps + row.k0;
                        const long long terms = row.hi - row.lo + 1;
                        if (st_rows) {                         // (the tile's rows all lie in [st_lo, st_lo + st_rows))
                            const double* x = staged + (row.lo - st_lo) * C + c;
                            for (long long i = 0; i < terms; ++i) { acc = fma(*x, *h, acc); x += C; h -= up; }
                        } else {
                            const double* x = src + k.soff + (row.lo - k.s0) * C + c;
                            for (long long i = 0; i < terms; ++i) { acc = fma(*x, *h, acc); x += C; h -= up; }
                        }
                    }
                }
                b[e] = from_f64_bits<KIND, LGS>(acc, raw_be != 0 && be);
                if (be) b[e] = rs_swap_elem<LGS>(b[e]);
                if (!vec && live) rs_store_elem<LGS>(out + ((i0 + e + k.shift * C) << LGS), b[e]);
                if (++c == C) { c = 0; ++s; }
            }
            if (vec) FRAD_NT_STORE(rs_pack16<LGS>(b), FRAD_GPTR(v4u, at));
        }
        if (st_rows) __syncthreads();                          // the next tile of this block stages over these rows
    }
}

}  // namespace
}  // namespace frad

using namespace frad;

extern "C" {

int frad_clips_resample(const double* src, const int64_t* src_off, const int64_t* src_row0, const int32_t* src_rows, int64_t n_clips,
                        int32_t C, int32_t up, int32_t down, const double* taps, int32_t half_len, const int64_t* out_row0,
                        const int32_t* valid, const int64_t* dst_row, int32_t out_dtype, uint32_t flags, void* out, const int64_t* out_off,
                        int64_t out_rows, void* stream) {
    if (!valid_pcm_dtype(out_dtype) || n_clips < 0 || out_rows < 0 || C < 1 || up < 1 || down < 1) return FRAD_E_INVALID;
    if ((long long)half_len != 10LL * (up > down ? up : down)) return FRAD_E_INVALID;
    if (n_clips == 0 || out_rows == 0) return FRAD_OK;
    if (!src_off || !src_row0 || !src_rows || !taps || !out_row0 || !valid || !out_off || !out) return FRAD_E_INVALID;
    const int kind = out_dtype >> 3, lg = (out_dtype >> 1) & 3, be = out_dtype & 1, raw = (flags & FRAD_RAW_BE_INTS) ? 1 : 0;
    // K: as many 256-store steps per tile as keep the source rows of a tile inside one clip within the LDS budget -- a tile of
    // R output rows reads about R * down / up + 2 * half / up + 2 source rows of C doubles
    const long long per_step = 256LL * (16 >> lg);
    int K = RS_K_MAX;
    for (; K > 1; --K) {
        const long long rows = (per_step * K + C - 1) / C + 1;
        const long long need = (rows * down + 2LL * half_len) / up + 3;
        if (need * C * 8 <= RS_LDS_BYTES) break;
    }
    const long long total = (long long)out_rows * C, per_block = per_step * K;
    long long blocks = (total + per_block - 1) / per_block;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* o = static_cast<unsigned char*>(out);
    const RsTables t{src_off, src_row0, src_rows, out_row0, valid, dst_row, out_off};
#define GO(KD, L) do { hipLaunchKernelGGL((k_clips_resample<KD, L>), grid, blk, (size_t)RS_LDS_BYTES, s, src, t, (long long)n_clips, (int)C, \
                                          (int)up, (int)down, taps, (int)half_len, o, (long long)out_rows, be, raw, K); } while (0)
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
