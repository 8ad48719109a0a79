// frad_epilogue.hip -- the decoder's output conversion (from_f64) and the native frame-header scan.
//
//   from_f64          backend/pcmformat.py:49-62, applied by the reference's caller right after every decode
//                     (src/decoder.py:23: from_f64(pcm, fmt).astype(fmt)): floats are cast (round to nearest even),
//                     integers are scaled by 2^(w-1) -- unsigned ones after adding 1 -- and TRUNCATED by numpy's astype.
//                     Out-of-range samples (a lossy decode overshoots +-1 now and then) are undefined in C; what numpy
//                     does on x86-64 is what cvttsd2si does, and that is reproduced here: 8/16-bit targets take the low
//                     bits of the 32-bit conversion, 32-bit unsigned the low half of the 64-bit one, an overflowing
//                     conversion yields the "integer indefinite" 0x80..0 (NaN too).
//   k_from_f64        float64 [n] -> any of the 20 PCM formats; fused into the profile-4 unpack (k_p4_unpack_pcm).
//   k_clips_ola       Decoder.overlap + flush() for many clips in one launch, ragged output (frad_clips_overlap_add).
//   k_clips_win       k_clips_ola on a row range of every clip, zero-padded and scattered into a dense batch
//                     (frad_clips_window_add: sample windows, window.py).
//   k_clips_carry     k_clips_ola for clips that are pieces of live streams: each starts from a carried fragment and ends in
//                     one (frad_clips_carry_add: DecoderPool, pool.py).
//   k_clips_cut       the Encoder's frame cut for many clips in one launch: fixed-length rows gathered from one buffer
//                     (frad_clips_frame_cut).
//   k_clips_carry_cut k_clips_cut for clips that are pieces of live streams: rows gathered from a carried remainder and the
//                     chunk that just arrived, and the next remainder written (frad_clips_carry_cut: EncoderPool, pool.py).
//   frad_asfh_scan   host code: walks a FrAD byte stream once and fills a table of frames (tools/asfh.py:98-134,
//                     decoder.py:82-106) so that the Python decoder no longer parses headers frame by frame.
#include <atomic>
#include "frad_p1.hpp"
#include "frad_launch.hpp"
#include "../../include/frad_hip.h"

#include <cmath>
#include <cstring>

namespace frad {
namespace {

template <int LGS> __device__ __forceinline__ u64 swap_elem(u64 b) {
    if constexpr (LGS == 1) return bswap16((uint32_t)b);
    else if constexpr (LGS == 2) return bswap32((uint32_t)b);
    else if constexpr (LGS == 3) return bswap64(b);
    else return b;
}
template <int LGS> __device__ __forceinline__ void store_elem(unsigned char* p, u64 b) {
    if constexpr (LGS == 0) *FRAD_GPTR(unsigned char, p) = (unsigned char)b;
    else if constexpr (LGS == 1) *FRAD_GPTR(unsigned short, p) = (unsigned short)b;
    else if constexpr (LGS == 2) *FRAD_GPTR(uint32_t, p) = (uint32_t)b;
    else *FRAD_GPTR(u64, p) = b;
}

// SRC 0: float64 samples at `in`; SRC 1: profile-4 payload rows (unpack + scrub fused, profile4.py:43-63)
template <int KIND, int LGS, int SRC>
__global__ void __launch_bounds__(256) k_from_f64(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, long long n, int be, Geom g) {
    constexpr int EPT = 16 >> LGS;                             // elements per thread: one 16-byte store when aligned
    const long long NC = (long long)g.N * g.C;
    const bool le = g.le && (g.bits % 8 == 0);
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * EPT; i0 < n; i0 += (long long)gridDim.x * blockDim.x * EPT) {
        u64 b[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const long long i = i0 + e;
            double x = 0.0;
            if (i < n) {
                if constexpr (SRC == 0) x = reinterpret_cast<const double*>(in)[i];
                else { const long long f = i / NC; x = code_to_f64(code_from_bytes(in + f * g.payload_stride, i - f * NC, g.bits, le), g.bits); }
            }
            b[e] = from_f64_bits<KIND, LGS>(x, g.raw_be != 0 && be);
            if (be) b[e] = swap_elem<LGS>(b[e]);
        }
        if (vec && i0 + EPT <= n) {
            v4u q = {0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                if constexpr (LGS == 3) { q[2 * e] = (uint32_t)b[e]; q[2 * e + 1] = (uint32_t)(b[e] >> 32); }
                else if constexpr (LGS == 2) q[e] = (uint32_t)b[e];
                else if constexpr (LGS == 1) q[e >> 1] |= (uint32_t)b[e] << (16 * (e & 1));
                else q[e >> 2] |= (uint32_t)b[e] << (8 * (e & 3));
            }
            FRAD_NT_STORE(q, FRAD_GPTR(v4u, out + (i0 << LGS)));
        } else {
#pragma unroll
            for (int e = 0; e < EPT; ++e) if (i0 + e < n) store_elem<LGS>(out + ((i0 + e) << LGS), b[e]);
        }
    }
}

// the decoder's overlap-add (k_p1_ola) with the output conversion applied on the way out: one pass over the decoded frames
// instead of two (decoder.py:28-46, then src/decoder.py:23 from_f64(...).astype(fmt))
template <int KIND, int LGS>
__global__ void __launch_bounds__(256) k_p1_ola_pcm(const double* __restrict__ frames, long long n_frames, int N, int C, int cut,
                                                    const double* __restrict__ prev_tail, const double* __restrict__ win,
                                                    unsigned char* __restrict__ out, double* __restrict__ next_tail, int be, int raw_be) {
    constexpr int EPT = 16 >> LGS;
    const long long n = n_frames * (long long)cut * C;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * EPT; i0 < n; i0 += (long long)gridDim.x * blockDim.x * EPT) {
        u64 b[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const double x = i0 + e < n ? p1_ola_value(frames, prev_tail, win, N, C, cut, i0 + e) : 0.0;
            b[e] = from_f64_bits<KIND, LGS>(x, raw_be != 0 && be);
            if (be) b[e] = swap_elem<LGS>(b[e]);
        }
        if (vec && i0 + EPT <= n) {
            v4u q = {0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                if constexpr (LGS == 3) { q[2 * e] = (uint32_t)b[e]; q[2 * e + 1] = (uint32_t)(b[e] >> 32); }
                else if constexpr (LGS == 2) q[e] = (uint32_t)b[e];
                else if constexpr (LGS == 1) q[e >> 1] |= (uint32_t)b[e] << (16 * (e & 1));
                else q[e >> 2] |= (uint32_t)b[e] << (8 * (e & 3));
            }
            FRAD_NT_STORE(q, FRAD_GPTR(v4u, out + (i0 << LGS)));
        } else {
#pragma unroll
            for (int e = 0; e < EPT; ++e) if (i0 + e < n) store_elem<LGS>(out + ((i0 + e) << LGS), b[e]);
        }
    }
    const int L = N - cut;
    if (next_tail != nullptr && n_frames > 0)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)L * C; i += (long long)gridDim.x * blockDim.x)
            next_tail[i] = frames[((n_frames - 1) * N + cut) * C + i];
}

// One output row of the clip-aware overlap-add: where row r of a clip (of m * cut + tail rows, or + L flush rows) comes from.
// Decoder.overlap + flush() (decoder.py:28-46, 110-114) per clip: the equal-length frames cross-fade as p1_ola_value does (same
// operation order, the same weights: `hann` = hann_table(L)), the clip's first frame is not faded, a last frame of another length
// is faded over its first L rows and written whole, and without one the last frame's rows [cut, N) follow unfaded.  `tail_win`
// (optional, hanning_in_overlap(L) as the caller computes it): the weights of a last frame whose own overlap length differs from
// L -- the frame the Decoder cross-fades on the host, in numpy, because the carried fragment has another geometry
// (decoder.py:207-209).
struct ClipRow {
    const double* src;                                         // the row's C samples
    const double* prev;                                        // the row it is faded against, or nullptr
    double w_in, w_out;
};
struct ClipCur {                                               // the clip a lane is in: its tables' entries, read once per clip
    long long j, base, end, f0, m, toff;
    int rows;
};

__device__ __forceinline__ ClipRow clips_ola_row(const double* __restrict__ frames, int N, int C, int cut, int ratio,
                                                 const double* __restrict__ tails, const double* __restrict__ tail_win,
                                                 const double* __restrict__ hann, const ClipCur& k, long long r) {
    const int L = N - cut;
    const long long body = k.m * cut;
    ClipRow o;
    o.prev = nullptr; o.w_in = 1.0; o.w_out = 0.0;
    bool table = false;
    int n;
    if (r < body) {
        long long f;
        if (r <= 0x7fffffffLL) { f = (uint32_t)r / (uint32_t)cut; n = (int)((uint32_t)r - (uint32_t)f * (uint32_t)cut); }
        else { f = r / cut; n = (int)(r - f * cut); }
        o.src = frames + ((k.f0 + f) * N + n) * C;
        if (n < L && f > 0) o.prev = frames + ((k.f0 + f - 1) * N + cut + n) * C;
    } else {
        const long long t = r - body;
        n = t < L ? (int)t : L;
        if (k.rows > 0) {
            o.src = tails + k.toff + t * C;
            if (t < L && k.m > 0) {
                o.prev = frames + ((k.f0 + k.m - 1) * N + cut + n) * C;
                table = tail_win != nullptr && k.rows - (int)((long long)k.rows * (ratio - 1) / ratio) != L;
            }
        } else {
            o.src = frames + ((k.f0 + k.m - 1) * N + cut + t) * C;       // the flush fragment
        }
    }
    if (o.prev != nullptr) {
        const double* w = table ? tail_win : hann;
        o.w_in = w[n]; o.w_out = w[L - 1 - n];
    }
    return o;
}

// frad_clips_overlap_add: a streaming pass over the ragged output.  A block owns a tile of CLIPS_K * 256 stores of 16 bytes, a
// lane every 256th of them.  The lane finds the clip of its first sample-frame by a binary search over out_off (the table
// stays in L2), keeps the clip's table entries in registers and searches again only when a store has left the clip, so no
// element searches from the start; where a row comes from and its two Hann weights are worked out once per row, not per
// sample.  Every decoded row is read once (a frame's last L rows only by the fade of the next frame, or as the flush fragment)
// and every output sample written once, 16 bytes per lane where the output allows it.
constexpr int CLIPS_K = 4;
template <int KIND, int LGS>
__global__ void __launch_bounds__(256) k_clips_ola(const double* __restrict__ frames, const int64_t* __restrict__ clip_frame0, long long n_clips,
                                                   int N, int C, int cut, int ratio, const double* __restrict__ tails,
                                                   const int64_t* __restrict__ tail_off, const int32_t* __restrict__ tail_rows,
                                                   const double* __restrict__ tail_win, const double* __restrict__ hann,
                                                   unsigned char* __restrict__ out, const int64_t* __restrict__ out_off, long long out_rows,
                                                   int be, int raw_be) {
    constexpr int EPT = 16 >> LGS;
    long long last = out_off[n_clips];
    if (last > out_rows) last = out_rows;                      // never beyond what the caller sized
    const long long n = last * C, n0 = (long long)out_off[0] * C;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const long long tile = 256LL * EPT * CLIPS_K;
    auto enter = [&](ClipCur& k, long long j) {
        k.j = j; k.base = out_off[j]; k.end = out_off[j + 1];
        k.f0 = clip_frame0[j]; k.m = clip_frame0[j + 1] - k.f0; k.rows = tail_rows[j]; k.toff = tail_off[j];
    };
    for (long long t0 = (long long)blockIdx.x * tile; t0 < n; t0 += (long long)gridDim.x * tile) {
        ClipCur k;
        k.j = -1; k.end = 0;
        for (int it = 0; it < CLIPS_K; ++it) {
            const long long i0 = t0 + ((long long)it * 256 + threadIdx.x) * EPT;
            if (i0 >= n) break;
            long long s;
            if (n <= 0x7fffffffLL) s = (uint32_t)i0 / (uint32_t)C; else s = i0 / C;
            int c = (int)(i0 - s * C);
            if (k.j < 0 || s >= k.end) {                       // the last clip that starts at or before sample-frame s
                long long lo = k.j < 0 ? 0 : k.j, hi = n_clips;
                while (hi - lo > 1) {
                    const long long mid = (lo + hi) >> 1;
                    if ((long long)out_off[mid] <= s) lo = mid; else hi = mid;
                }
                enter(k, lo);
            }
            ClipRow row;
            row.src = nullptr; row.prev = nullptr; row.w_in = 1.0; row.w_out = 0.0;
            u64 b[EPT];
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                double x = 0.0;
                if (i0 + e < n && i0 + e >= n0) {
                    if (row.src == nullptr || c == 0) {
                        while (s >= k.end && k.j + 1 < n_clips) enter(k, k.j + 1);
                        row = clips_ola_row(frames, N, C, cut, ratio, tails, tail_win, hann, k, s - k.base);
                    }
                    x = row.src[c];
                    if (row.prev != nullptr) {
                        x = x * row.w_in;
                        x = x + row.prev[c] * row.w_out;
                    }
                }
                b[e] = from_f64_bits<KIND, LGS>(x, raw_be != 0 && be);
                if (be) b[e] = swap_elem<LGS>(b[e]);
                if (++c == C) { c = 0; ++s; }
            }
            if (vec && i0 + EPT <= n && i0 >= n0) {
                v4u q = {0, 0, 0, 0};
#pragma unroll
                for (int e = 0; e < EPT; ++e) {
                    if constexpr (LGS == 3) { q[2 * e] = (uint32_t)b[e]; q[2 * e + 1] = (uint32_t)(b[e] >> 32); }
                    else if constexpr (LGS == 2) q[e] = (uint32_t)b[e];
                    else if constexpr (LGS == 1) q[e >> 1] |= (uint32_t)b[e] << (16 * (e & 1));
                    else q[e >> 2] |= (uint32_t)b[e] << (8 * (e & 3));
                }
                FRAD_NT_STORE(q, FRAD_GPTR(v4u, out + (i0 << LGS)));
            } else {
#pragma unroll
                for (int e = 0; e < EPT; ++e) if (i0 + e < n && i0 + e >= n0) store_elem<LGS>(out + ((i0 + e) << LGS), b[e]);
            }
        }
    }
}

// frad_clips_window_add: k_clips_ola's pass, evaluated on rows [skip, skip + valid) of every clip's timeline and written to a
// span that may lie anywhere in `out`.  The launch is partitioned by out_off exactly as above (a lane owns 16-byte stores of the
// partition, searches out_off only when a store has left the clip, one clips_ola_row per row), and the row's sources and
// weights are clips_ola_row's at timeline row skip + r, so a window is bit for bit the slice of the whole clip.  Rows from
// `valid` to the end of the span are the conversion of 0.0.  With dst_row the span of clip j starts at sample-frame dst_row[j]
// of `out` instead of out_off[j], so the address of a store is the clip's: whether it leaves as 16 bytes is decided per store,
// from that address and from the store lying inside one span (without dst_row the spans follow each other and a store may
// straddle two, as above); every other store goes element by element, and nothing outside the spans is written.
struct WinCur : ClipCur {
    long long skip, shift;                                     // shift: the span's first sample-frame in `out` less out_off[j]
    int valid;
};
template <int LGS> __device__ __forceinline__ v4u pack16(const u64* b) {
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
struct WinTables {                                             // the per-clip tables of frad_clips_window_add (device memory)
    const int64_t* clip_f0; const int32_t* clip_m; const int64_t* tail_off; const int32_t* tail_rows;
    const int64_t* skip; const int32_t* valid; const int64_t* dst_row; const int64_t* out_off;
};
template <int KIND, int LGS>
__global__ void __launch_bounds__(256) k_clips_win(const double* __restrict__ frames, WinTables t, long long n_clips, int N, int C, int cut,
                                                   int ratio, const double* __restrict__ tails, const double* __restrict__ tail_win,
                                                   const double* __restrict__ hann, unsigned char* __restrict__ out, long long out_rows,
                                                   int be, int raw_be) {
    constexpr int EPT = 16 >> LGS;
    long long last = t.out_off[n_clips];
    if (last > out_rows) last = out_rows;                      // never beyond what the caller sized
    const long long n = last * C, n0 = (long long)t.out_off[0] * C;
    const long long tile = 256LL * EPT * CLIPS_K;
    auto enter = [&](WinCur& k, long long j) {
        k.j = j; k.base = t.out_off[j]; k.end = t.out_off[j + 1];
        k.f0 = t.clip_f0[j]; k.m = t.clip_m[j]; k.rows = t.tail_rows[j]; k.toff = t.tail_off[j];
        k.skip = t.skip[j]; k.valid = t.valid[j];
        k.shift = t.dst_row != nullptr ? (long long)t.dst_row[j] - k.base : 0;
    };
    for (long long t0 = (long long)blockIdx.x * tile; t0 < n; t0 += (long long)gridDim.x * tile) {
        WinCur k;
        k.j = -1; k.end = 0;
        for (int it = 0; it < CLIPS_K; ++it) {
            const long long i0 = t0 + ((long long)it * 256 + threadIdx.x) * EPT;
            if (i0 >= n) break;
            long long s;
            if (n <= 0x7fffffffLL) s = (uint32_t)i0 / (uint32_t)C; else s = i0 / C;
            int c = (int)(i0 - s * C);
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
            const long long s_last = s + (uint32_t)(c + EPT - 1) / (uint32_t)C;
            unsigned char* const at = out + ((i0 + k.shift * C) << LGS);
            const bool vec = i0 >= n0 && i0 + EPT <= n && (t.dst_row == nullptr || s_last < k.end) &&
                             (reinterpret_cast<uintptr_t>(at) & 15) == 0;
            ClipRow row;
            row.src = nullptr; row.prev = nullptr; row.w_in = 1.0; row.w_out = 0.0;
            bool have = false, pad = false;
            u64 b[EPT];
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const bool live = i0 + e < n && i0 + e >= n0;
                double x = 0.0;
                if (live) {
                    if (!have || c == 0) {
                        while (s >= k.end && k.j + 1 < n_clips) enter(k, k.j + 1);
                        const long long r = s - k.base;
                        pad = r >= k.valid;
                        if (!pad) row = clips_ola_row(frames, N, C, cut, ratio, tails, tail_win, hann, k, k.skip + r);
                        have = true;
                    }
                    if (!pad) {
                        x = row.src[c];
                        if (row.prev != nullptr) {
                            x = x * row.w_in;
                            x = x + row.prev[c] * row.w_out;
                        }
                    }
                }
                b[e] = from_f64_bits<KIND, LGS>(x, raw_be != 0 && be);
                if (be) b[e] = swap_elem<LGS>(b[e]);
                if (!vec && live) store_elem<LGS>(out + ((i0 + e + k.shift * C) << LGS), b[e]);
                if (++c == C) { c = 0; ++s; }
            }
            if (vec) FRAD_NT_STORE(pack16<LGS>(b), FRAD_GPTR(v4u, at));
        }
    }
}

// frad_clips_carry_add: k_clips_ola's pass for clips that are the next piece of a live stream.  A clip is m whole frames and
// nothing else (no last frame of another length, no flush fragment): its first frame is faded against the fragment the stream
// carried in (prev_ptr[j], when there is one), and rows [cut, N) of its last frame leave as the fragment it carries out
// (next_ptr[j], float64 whatever the output format).  The launch is partitioned by out_off as above (a lane owns 16-byte
// stores, searches out_off only when a store has left the clip, one row lookup per row); the weights and the operation order
// are p1_ola_value's, so a clip's rows are frad_p1_overlap_add_pcm's bits.  The fragments are copied by a second grid-stride
// loop over n_clips * L * C elements; a clip without frames is skipped by both loops, so its pending fragment stays pending.
struct CarryCur {                                              // the clip a lane is in
    long long j, base, end, f0;
    const double* prev;
};
template <int KIND, int LGS>
__global__ void __launch_bounds__(256) k_clips_carry(const double* __restrict__ frames, const int64_t* __restrict__ clip_frame0, long long n_clips,
                                                     int N, int C, int cut, const double* const* __restrict__ prev_ptr,
                                                     double* const* __restrict__ next_ptr, const double* __restrict__ hann,
                                                     unsigned char* __restrict__ out, const int64_t* __restrict__ out_off, long long out_rows,
                                                     int be, int raw_be) {
    constexpr int EPT = 16 >> LGS;
    const int L = N - cut;
    long long last = out_off[n_clips];
    if (last > out_rows) last = out_rows;                      // never beyond what the caller sized
    const long long n = last * C, n0 = (long long)out_off[0] * C;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const long long tile = 256LL * EPT * CLIPS_K;
    auto enter = [&](CarryCur& k, long long j) {
        k.j = j; k.base = out_off[j]; k.end = out_off[j + 1];
        k.f0 = clip_frame0[j]; k.prev = (L > 0 && prev_ptr != nullptr) ? prev_ptr[j] : nullptr;
    };
    for (long long t0 = (long long)blockIdx.x * tile; t0 < n; t0 += (long long)gridDim.x * tile) {
        CarryCur k;
        k.j = -1; k.end = 0;
        for (int it = 0; it < CLIPS_K; ++it) {
            const long long i0 = t0 + ((long long)it * 256 + threadIdx.x) * EPT;
            if (i0 >= n) break;
            long long s;
            if (n <= 0x7fffffffLL) s = (uint32_t)i0 / (uint32_t)C; else s = i0 / C;
            int c = (int)(i0 - s * C);
            if (k.j < 0 || s >= k.end) {                       // the last clip that starts at or before sample-frame s
                long long lo = k.j < 0 ? 0 : k.j, hi = n_clips;
                while (hi - lo > 1) {
                    const long long mid = (lo + hi) >> 1;
                    if ((long long)out_off[mid] <= s) lo = mid; else hi = mid;
                }
                enter(k, lo);
            }
            ClipRow row;
            row.src = nullptr; row.prev = nullptr; row.w_in = 1.0; row.w_out = 0.0;
            u64 b[EPT];
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                double x = 0.0;
                if (i0 + e < n && i0 + e >= n0) {
                    if (row.src == nullptr || c == 0) {
                        while (s >= k.end && k.j + 1 < n_clips) enter(k, k.j + 1);
                        const long long r = s - k.base;
                        long long f;
                        int nn;
                        if (r <= 0x7fffffffLL) { f = (uint32_t)r / (uint32_t)cut; nn = (int)((uint32_t)r - (uint32_t)f * (uint32_t)cut); }
                        else { f = r / cut; nn = (int)(r - f * cut); }
                        row.src = frames + ((k.f0 + f) * N + nn) * C;
                        row.prev = nullptr;
                        if (nn < L) {
                            if (f > 0) row.prev = frames + ((k.f0 + f - 1) * N + cut + nn) * C;
                            else if (k.prev != nullptr) row.prev = k.prev + (long long)nn * C;
                            if (row.prev != nullptr) { row.w_in = hann[nn]; row.w_out = hann[L - 1 - nn]; }
                        }
                    }
                    x = row.src[c];
                    if (row.prev != nullptr) {
                        x = x * row.w_in;
                        x = x + row.prev[c] * row.w_out;
                    }
                }
                b[e] = from_f64_bits<KIND, LGS>(x, raw_be != 0 && be);
                if (be) b[e] = swap_elem<LGS>(b[e]);
                if (++c == C) { c = 0; ++s; }
            }
            if (vec && i0 + EPT <= n && i0 >= n0) {
                FRAD_NT_STORE(pack16<LGS>(b), FRAD_GPTR(v4u, out + (i0 << LGS)));
            } else {
#pragma unroll
                for (int e = 0; e < EPT; ++e) if (i0 + e < n && i0 + e >= n0) store_elem<LGS>(out + ((i0 + e) << LGS), b[e]);
            }
        }
    }
    if (L > 0 && next_ptr != nullptr) {                        // the fragments carried out: plain copies, bits unchanged
        const long long per = (long long)L * C, total = n_clips * per;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
            long long j;
            if (total <= 0x7fffffffLL) j = (uint32_t)i / (uint32_t)per; else j = i / per;
            const long long e = i - j * per;
            const long long f0 = clip_frame0[j], m = clip_frame0[j + 1] - f0;
            double* const dst = next_ptr[j];
            if (m > 0 && dst != nullptr) dst[e] = frames[((f0 + m - 1) * N + cut) * C + e];
        }
    }
}

// frad_clips_frame_cut: frad_clips_overlap_add turned round -- the encoder's frame cut for many clips, a streaming pass over
// the fixed-length output rows.  A block owns a tile of CUT_K * 256 chunks of 16 output bytes, a lane every 256th of them; the
// chunks sit at 16-byte aligned ADDRESSES (chunk c covers output bytes [16 c - head, 16 c - head + 16), head = out mod 16), so
// that only the first and the last chunk of the whole output can be partial.  A chunk finds its row by one division of its
// byte offset by the row's byte length -- no search, no scratch, and rows of a few bytes share a lane instead of taking a
// block each.  A chunk that lies inside one row, and there wholly inside the valid bytes or wholly inside the padding, is one
// 16-byte load from wherever the source row starts (global memory takes the unaligned address) or none, and one 16-byte
// store; a chunk that straddles rows, or the end of a row's valid bytes, is put together byte by byte in registers and still
// leaves as one store.  Only the two partial chunks store bytes.  The stores are plain, not nontemporal: the transform that
// follows reads the block at once, and a plain store leaves the line in L2.
constexpr int CUT_K = 4;
__device__ __forceinline__ v4u load16_anywhere(const unsigned char* p) {
    v4u q;
    __builtin_memcpy(&q, p, 16);
    return q;
}
__global__ void __launch_bounds__(256) k_clips_cut(const unsigned char* __restrict__ src, const int64_t* __restrict__ row_src,
                                                   const int32_t* __restrict__ row_valid, long long n_rows, long long rb, int step,
                                                   unsigned char* __restrict__ out) {
    const long long total = n_rows * rb;
    const long long head = (long long)(reinterpret_cast<uintptr_t>(out) & 15);
    const long long n_chunks = (total + head + 15) >> 4;
    const bool small = total + 16 <= 0xffffffffLL;
    const long long tile = 256LL * CUT_K;
    for (long long c0 = (long long)blockIdx.x * tile; c0 < n_chunks; c0 += (long long)gridDim.x * tile) {
#pragma unroll 1
        for (int it = 0; it < CUT_K; ++it) {                   // (not unrolled: the branches below keep the steps apart anyway)
            const long long c = c0 + (long long)it * 256 + threadIdx.x;
            if (c >= n_chunks) break;
            const long long o = 16 * c - head;                 // < 0 only for chunk 0 of a misaligned output
            const long long lo = o < 0 ? 0 : o, hi = o + 16 > total ? total : o + 16;
            long long r = small ? (long long)((uint32_t)lo / (uint32_t)rb) : lo / rb;
            long long w = lo - r * rb;                         // the chunk's first byte inside row r
            long long vb = (long long)row_valid[r] * step;     // the row's valid bytes, never more than the row
            vb = vb < 0 ? 0 : (vb > rb ? rb : vb);
            const unsigned char* s = src + row_src[r] * step;
            v4u q = {0, 0, 0, 0};
            if (hi - lo == 16 && w + 16 <= rb && (w + 16 <= vb || w >= vb)) {
                if (w < vb) q = load16_anywhere(s + w);
                *FRAD_GPTR(v4u, out + o) = q;
                continue;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long long b = o + k;
                if (b < lo || b >= hi) continue;
                if (w == rb) {                                 // the next row (rb >= 1: at most one step per byte)
                    ++r; w = 0;
                    vb = (long long)row_valid[r] * step;
                    vb = vb < 0 ? 0 : (vb > rb ? rb : vb);
                    s = src + row_src[r] * step;
                }
                const uint32_t x = w < vb ? s[w] : 0u;
                q[k >> 2] |= x << (8 * (k & 3));
                ++w;
            }
            if (hi - lo == 16) *FRAD_GPTR(v4u, out + o) = q;
            else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (o + k >= lo && o + k < hi) out[o + k] = (unsigned char)(q[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

// frad_clips_carry_cut: k_clips_cut for clips that are pieces of live streams.  A clip's sample-frames are a virtual sequence V
// of two segments -- what the stream carried over from its last tick, then the chunk that just arrived (a span of one joined
// buffer) -- and every row is whole, so there is no padding.  The launch keeps k_clips_cut's shape: 16-byte stores at aligned
// addresses of `out`, one division finds a chunk's row, a chunk inside one segment of one row is one unaligned 16-byte load and
// one store, and only a chunk that straddles a row end or the seam is put together byte by byte.  Behind the rows the same
// launch copies every clip's remainder V[next_at, have) to next_ptr[j]: a block takes every gridDim.x-th clip and moves it the
// same way (aligned 16-byte stores, byte edges) -- the pool keeps a remainder below one row, so a clip is a few KiB at most.
struct CarrySeg {                                              // V[p] = p < cb ? carry[p] : chunk[p - cb], p in bytes
    const unsigned char* carry;
    const unsigned char* chunk;
    long long cb;
};
__device__ __forceinline__ uint32_t seg_byte(const CarrySeg& s, long long p) { return p < s.cb ? s.carry[p] : s.chunk[p - s.cb]; }
__device__ __forceinline__ v4u seg_load16(const CarrySeg& s, long long p) {      // V[p, p + 16), all of it inside V
    if (p + 16 <= s.cb) return load16_anywhere(s.carry + p);
    if (p >= s.cb) return load16_anywhere(s.chunk + (p - s.cb));
    v4u q = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) q[k >> 2] |= seg_byte(s, p + k) << (8 * (k & 3));
    return q;
}
__global__ void __launch_bounds__(256) k_clips_carry_cut(const unsigned char* const* __restrict__ carry_ptr, const int32_t* __restrict__ carry_len,
                                                         const unsigned char* __restrict__ src, const int64_t* __restrict__ src_off,
                                                         long long n_clips, const int32_t* __restrict__ row_clip,
                                                         const int64_t* __restrict__ row_at, long long n_rows, long long rb, int step,
                                                         unsigned char* __restrict__ out, const int64_t* __restrict__ next_at,
                                                         unsigned char* const* __restrict__ next_ptr) {
    auto seg_of = [&](long long j) {
        CarrySeg s;
        s.cb = (long long)carry_len[j] * step;
        s.carry = s.cb > 0 ? carry_ptr[j] : nullptr;
        s.chunk = src + src_off[j] * step;
        return s;
    };
    const long long total = n_rows * rb;
    const long long head = (long long)(reinterpret_cast<uintptr_t>(out) & 15);
    const long long n_chunks = total > 0 ? (total + head + 15) >> 4 : 0;
    const bool small = total + 16 <= 0xffffffffLL;
    const long long tile = 256LL * CUT_K;
    for (long long c0 = (long long)blockIdx.x * tile; c0 < n_chunks; c0 += (long long)gridDim.x * tile) {
#pragma unroll 1
        for (int it = 0; it < CUT_K; ++it) {
            const long long c = c0 + (long long)it * 256 + threadIdx.x;
            if (c >= n_chunks) break;
            const long long o = 16 * c - head;                 // < 0 only for chunk 0 of a misaligned output
            const long long lo = o < 0 ? 0 : o, hi = o + 16 > total ? total : o + 16;
            long long r = small ? (long long)((uint32_t)lo / (uint32_t)rb) : lo / rb;
            long long w = lo - r * rb;                         // the chunk's first byte inside row r
            CarrySeg s = seg_of(row_clip[r]);
            long long p = row_at[r] * step + w;                // ... and inside the clip's V
            if (hi - lo == 16 && w + 16 <= rb) {
                *FRAD_GPTR(v4u, out + o) = seg_load16(s, p);
                continue;
            }
            v4u q = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long long b = o + k;
                if (b < lo || b >= hi) continue;
                if (w == rb) {                                 // the next row (rb >= 1: at most one step per byte)
                    ++r; w = 0;
                    s = seg_of(row_clip[r]);
                    p = row_at[r] * step;
                }
                q[k >> 2] |= seg_byte(s, p) << (8 * (k & 3));
                ++w; ++p;
            }
            if (hi - lo == 16) *FRAD_GPTR(v4u, out + o) = q;
            else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (o + k >= lo && o + k < hi) out[o + k] = (unsigned char)(q[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
    if (next_ptr == nullptr) return;
    for (long long j = blockIdx.x; j < n_clips; j += gridDim.x) {      // the remainders: plain copies, bits unchanged
        unsigned char* const dst = next_ptr[j];
        if (dst == nullptr) continue;
        const CarrySeg s = seg_of(j);
        const long long p0 = next_at[j] * step;
        const long long n = s.cb + (src_off[j + 1] - src_off[j]) * step - p0;
        if (n <= 0) continue;
        long long hd = (16 - (long long)(reinterpret_cast<uintptr_t>(dst) & 15)) & 15;      // bytes in front of the first aligned store
        if (hd > n) hd = n;
        const long long nq = (n - hd) >> 4, edge = n - 16 * nq;                             // edge: hd in front, the rest behind (< 31)
        for (long long i = threadIdx.x; i < nq; i += blockDim.x) *FRAD_GPTR(v4u, dst + hd + 16 * i) = seg_load16(s, p0 + hd + 16 * i);
        for (long long i = threadIdx.x; i < edge; i += blockDim.x) {
            const long long at = i < hd ? i : 16 * nq + i;
            dst[at] = (unsigned char)seg_byte(s, p0 + at);
        }
    }
}

template <int SRC>
int launch_from_f64(int dtype, const unsigned char* in, unsigned char* out, long long n, const Geom& g, hipStream_t s) {
    const int kind = dtype >> 3, lg = (dtype >> 1) & 3, be = dtype & 1;
    const long long per_block = 256LL * (16 >> lg);
    long long blocks = (n + per_block - 1) / per_block;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), blk(256);
#define GO(K, L) hipLaunchKernelGGL((k_from_f64<K, L, SRC>), grid, blk, 0, s, in, out, n, be, g)
    switch (kind * 4 + lg) {
        case 0: GO(0, 0); break; case 1: GO(0, 1); break; case 2: GO(0, 2); break; case 3: GO(0, 3); break;
        case 4: GO(1, 0); break; case 5: GO(1, 1); break; case 6: GO(1, 2); break; case 7: GO(1, 3); break;
        case 9: GO(2, 1); break; case 10: GO(2, 2); break; case 11: GO(2, 3); break;
        default: return FRAD_E_INVALID;
    }
#undef GO
    return FRAD_OK;
}

}  // namespace
}  // namespace frad

using namespace frad;

// calls of frad_p{0,1}_digital_pcm that took the float64 scratch + second pass (diagnostic: tests assert which geometries still do)
static std::atomic<long long> g_second_passes{0};
extern "C" long long frad_debug_second_passes(void) { return g_second_passes.load(std::memory_order_relaxed); }

extern "C" {

int frad_from_f64(const double* pcm, int64_t n_values, int32_t out_dtype, uint32_t flags, void* out, void* stream) {
    if (n_values < 0 || !valid_pcm_dtype(out_dtype)) return FRAD_E_INVALID;
    if (n_values == 0) return FRAD_OK;
    if (!pcm || !out) return FRAD_E_INVALID;
    Geom g{}; g.N = 1; g.C = 1; g.bits = 64; g.raw_be = (flags & FRAD_RAW_BE_INTS) ? 1 : 0;
    const int rc = launch_from_f64<0>(out_dtype, reinterpret_cast<const unsigned char*>(pcm), static_cast<unsigned char*>(out), n_values, g,
                                      static_cast<hipStream_t>(stream));
    if (rc != FRAD_OK) return rc;
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

int frad_p4_digital_pcm(const void* payload, int64_t payload_stride, int64_t n_frames, int32_t N, int32_t C, int32_t bits,
                        uint32_t flags, int32_t out_dtype, void* pcm_out, void* stream) {
    if (n_frames < 0 || N < 1 || C < 1 || C > 256 || !valid_pcm_dtype(out_dtype)) return FRAD_E_INVALID;
    if (!valid_bits(bits)) return FRAD_E_INVALID;
    if (n_frames == 0) return FRAD_OK;
    if (!payload || !pcm_out || payload_stride < (int64_t)frad_payload_bytes(N, C, bits)) return FRAD_E_INVALID;
    Geom g{}; g.n_frames = n_frames; g.N = N; g.C = C; g.bits = bits; g.le = (flags & FRAD_LITTLE_ENDIAN) ? 1 : 0; g.payload_stride = payload_stride;
    g.raw_be = (flags & FRAD_RAW_BE_INTS) ? 1 : 0;
    const int rc = launch_from_f64<1>(out_dtype, static_cast<const unsigned char*>(payload), static_cast<unsigned char*>(pcm_out),
                                      (long long)n_frames * N * C, g, static_cast<hipStream_t>(stream));
    if (rc != FRAD_OK) return rc;
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

// profile 0 / 1: N = 2048 stereo at 16 / 32-bit storage converts inside the wave kernel's output stage; elsewhere the
// transform kernels write float64 and the narrowing pass follows on the same stream (stream-ordered scratch).
int frad_p0_digital_pcm(const void* payload, int64_t payload_stride, int64_t n_frames, int32_t N, int32_t C, int32_t bits,
                        uint32_t flags, int32_t out_dtype, void* pcm_out, void* stream) {
    if (!valid_pcm_dtype(out_dtype)) return FRAD_E_INVALID;
    if (out_dtype == FRAD_PCM_F64LE) return frad_p0_digital(payload, payload_stride, n_frames, N, C, bits, flags, static_cast<double*>(pcm_out), stream);
    if (n_frames < 0 || N < 1 || C < 1) return FRAD_E_INVALID;
    if (n_frames == 0) return FRAD_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (payload && pcm_out && (bits == 16 || bits == 32) && payload_stride >= (int64_t)frad_payload_bytes(N, C, bits)) {
        // N = 2048 stereo: the conversion is fused into the wave kernel's output stage (one pass, 4-6 B per sample out)
        Geom g{};
        g.n_frames = n_frames; g.frame_stride = N; g.payload_stride = payload_stride; g.N = N; g.C = C; g.bits = bits;
        g.le = (flags & FRAD_LITTLE_ENDIAN) ? 1 : 0; g.dtype = FRAD_PCM_F64LE; g.fpb = 1; g.n_valid = N; g.cg = C;
        const int ai = (aligned16(payload) && payload_stride % 16 == 0) ? 1 : 0;
        FRAD_TRY_LAUNCH(launch_p0_inv_wave_pcm(s, static_cast<const unsigned char*>(payload), pcm_out, g, ai, out_dtype));
    }
    {   // every other LDS-resident kernel converts in its own store (one pass, no scratch); only the unit / two-pass whole-row kernels'
        // geometries are rerouted to their one-shot twins for it, and frames wider than a CU keep the second pass
        const int r = p0_digital_out(payload, payload_stride, n_frames, N, C, bits, flags, out_dtype, pcm_out, stream);
        if (r != 1) return r;
    }
    g_second_passes.fetch_add(1, std::memory_order_relaxed);
    Scratch ws(s);
    const size_t n = (size_t)n_frames * N * C;
    int rc = ws.alloc(n * 8);
    if (rc != FRAD_OK) return rc;
    rc = frad_p0_digital(payload, payload_stride, n_frames, N, C, bits, flags, static_cast<double*>(ws.p), stream);
    if (rc != FRAD_OK) return rc;
    return frad_from_f64(static_cast<const double*>(ws.p), (int64_t)n, out_dtype, flags, pcm_out, stream);
}

int frad_p1_digital_pcm(const int32_t* q, const int32_t* tq, int64_t n_frames, int32_t N, int32_t C, int32_t bits, int32_t srate,
                        int32_t out_dtype, uint32_t flags, void* pcm_out, void* stream) {
    if (!valid_pcm_dtype(out_dtype)) return FRAD_E_INVALID;
    if (out_dtype == FRAD_PCM_F64LE) return frad_p1_digital(q, tq, n_frames, N, C, bits, srate, static_cast<double*>(pcm_out), stream);
    if (n_frames < 0 || N < 1 || C < 1) return FRAD_E_INVALID;
    if (n_frames == 0) return FRAD_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        const int r = p1_digital_out(q, tq, n_frames, N, C, bits, srate, out_dtype, flags, pcm_out, stream);   // one pass where the kernel's store converts
        if (r != 1) return r;
    }
    g_second_passes.fetch_add(1, std::memory_order_relaxed);
    Scratch ws(s);
    const size_t n = (size_t)n_frames * N * C;
    int rc = ws.alloc(n * 8);
    if (rc != FRAD_OK) return rc;
    rc = frad_p1_digital(q, tq, n_frames, N, C, bits, srate, static_cast<double*>(ws.p), stream);
    if (rc != FRAD_OK) return rc;
    return frad_from_f64(static_cast<const double*>(ws.p), (int64_t)n, out_dtype, flags, pcm_out, stream);
}

int frad_p1_overlap_add_pcm(const double* frames, int64_t n_frames, int32_t N, int32_t C, int32_t overlap_ratio, const double* prev_tail,
                            int32_t out_dtype, uint32_t flags, void* ola_out, double* next_tail, void* stream) {
    if (!valid_pcm_dtype(out_dtype)) return FRAD_E_INVALID;
    if (out_dtype == FRAD_PCM_F64LE) return frad_p1_overlap_add(frames, n_frames, N, C, overlap_ratio, prev_tail, static_cast<double*>(ola_out), next_tail, stream);
    if (n_frames < 0 || N < 1 || C < 1 || overlap_ratio < 2 || overlap_ratio > 256) return FRAD_E_INVALID;
    if (n_frames == 0) return FRAD_OK;
    if (!frames || !ola_out) return FRAD_E_INVALID;
    const int cut = (int)((long long)N * (overlap_ratio - 1) / overlap_ratio);     // decoder.py:44
    const int kind = out_dtype >> 3, lg = (out_dtype >> 1) & 3, be = out_dtype & 1, raw = (flags & FRAD_RAW_BE_INTS) ? 1 : 0;
    const long long total = n_frames * (long long)cut * C, per_block = 256LL * (16 >> lg);
    long long blocks = (total + per_block - 1) / per_block;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* o = static_cast<unsigned char*>(ola_out);
    const double* win = nullptr;
    if (const int rc = hann_table(N - cut, &win)) return rc;
#define GO(K, L) hipLaunchKernelGGL((k_p1_ola_pcm<K, L>), grid, blk, 0, s, frames, (long long)n_frames, N, C, cut, prev_tail, win, o, next_tail, be, raw)
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

int frad_clips_overlap_add(const double* frames, const int64_t* clip_frame0, int64_t n_clips, int32_t N, int32_t C, int32_t overlap_ratio,
                           const double* tails, const int64_t* tail_off, const int32_t* tail_rows, const double* tail_win,
                           int32_t out_dtype, uint32_t flags, void* out, const int64_t* out_off, int64_t out_rows, void* stream) {
    if (!valid_pcm_dtype(out_dtype) || n_clips < 0 || out_rows < 0 || N < 1 || C < 1) return FRAD_E_INVALID;
    if (overlap_ratio != 0 && (overlap_ratio < 2 || overlap_ratio > 256)) return FRAD_E_INVALID;
    if (n_clips == 0 || out_rows == 0) return FRAD_OK;
    if (!clip_frame0 || !tail_off || !tail_rows || !out_off || !out) return FRAD_E_INVALID;
    const int cut = overlap_ratio ? (int)((long long)N * (overlap_ratio - 1) / overlap_ratio) : N;     // decoder.py:44
    const int ratio = overlap_ratio ? overlap_ratio : 1;
    const int kind = out_dtype >> 3, lg = (out_dtype >> 1) & 3, be = out_dtype & 1, raw = (flags & FRAD_RAW_BE_INTS) ? 1 : 0;
    const long long total = (long long)out_rows * C, per_block = 256LL * (16 >> lg) * CLIPS_K;
    long long blocks = (total + per_block - 1) / per_block;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* o = static_cast<unsigned char*>(out);
    const double* hann = nullptr;                              // (no overlap: cut = N and nothing is faded)
    if (N > cut) if (const int rc = hann_table(N - cut, &hann)) return rc;
#define GO(K, L) hipLaunchKernelGGL((k_clips_ola<K, L>), grid, blk, 0, s, frames, clip_frame0, (long long)n_clips, N, C, cut, ratio, tails, \
                                    tail_off, tail_rows, tail_win, hann, o, out_off, (long long)out_rows, be, raw)
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

int frad_clips_window_add(const double* frames, const int64_t* clip_f0, const int32_t* clip_m, int64_t n_clips, int32_t N, int32_t C,
                          int32_t overlap_ratio, const double* tails, const int64_t* tail_off, const int32_t* tail_rows, const double* tail_win,
                          const int64_t* skip, const int32_t* valid, const int64_t* dst_row, int32_t out_dtype, uint32_t flags, void* out,
                          const int64_t* out_off, int64_t out_rows, void* stream) {
    if (!valid_pcm_dtype(out_dtype) || n_clips < 0 || out_rows < 0 || N < 1 || C < 1) return FRAD_E_INVALID;
    if (overlap_ratio != 0 && (overlap_ratio < 2 || overlap_ratio > 256)) return FRAD_E_INVALID;
    if (n_clips == 0 || out_rows == 0) return FRAD_OK;
    if (!clip_f0 || !clip_m || !tail_off || !tail_rows || !skip || !valid || !out_off || !out) return FRAD_E_INVALID;
    const int cut = overlap_ratio ? (int)((long long)N * (overlap_ratio - 1) / overlap_ratio) : N;     // decoder.py:44
    const int ratio = overlap_ratio ? overlap_ratio : 1;
    const int kind = out_dtype >> 3, lg = (out_dtype >> 1) & 3, be = out_dtype & 1, raw = (flags & FRAD_RAW_BE_INTS) ? 1 : 0;
    const long long total = (long long)out_rows * C, per_block = 256LL * (16 >> lg) * CLIPS_K;
    long long blocks = (total + per_block - 1) / per_block;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* o = static_cast<unsigned char*>(out);
    const WinTables t{clip_f0, clip_m, tail_off, tail_rows, skip, valid, dst_row, out_off};
    const double* hann = nullptr;                              // (no overlap: cut = N and nothing is faded)
    if (N > cut) if (const int rc = hann_table(N - cut, &hann)) return rc;
#define GO(K, L) hipLaunchKernelGGL((k_clips_win<K, L>), grid, blk, 0, s, frames, t, (long long)n_clips, N, C, cut, ratio, tails, tail_win, hann, o, \
                                    (long long)out_rows, be, raw)
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

int frad_clips_carry_add(const double* frames, const int64_t* clip_frame0, int64_t n_clips, int32_t N, int32_t C, int32_t overlap_ratio,
                         const double* const* prev_ptr, double* const* next_ptr, int32_t out_dtype, uint32_t flags, void* out,
                         const int64_t* out_off, int64_t out_rows, void* stream) {
    if (n_clips < 0 || out_rows < 0) return FRAD_E_INVALID;
    if (n_clips == 0) return FRAD_OK;
    if (!valid_pcm_dtype(out_dtype) || N < 1 || C < 1) return FRAD_E_INVALID;
    if (overlap_ratio != 0 && (overlap_ratio < 2 || overlap_ratio > 256)) return FRAD_E_INVALID;
    if (out_rows == 0) return FRAD_OK;                         // every clip is empty: no rows, and no fragment changes hands
    if (!frames || !clip_frame0 || !out_off || !out) return FRAD_E_INVALID;
    const int cut = overlap_ratio ? (int)((long long)N * (overlap_ratio - 1) / overlap_ratio) : N;     // decoder.py:44
    if (cut < 1) return FRAD_E_INVALID;                        // (N = 1 with a ratio: a frame that keeps no row cannot own out_rows > 0)
    const int kind = out_dtype >> 3, lg = (out_dtype >> 1) & 3, be = out_dtype & 1, raw = (flags & FRAD_RAW_BE_INTS) ? 1 : 0;
    const long long total = (long long)out_rows * C, per_block = 256LL * (16 >> lg) * CLIPS_K;
    long long blocks = (total + per_block - 1) / per_block;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* o = static_cast<unsigned char*>(out);
    const double* hann = nullptr;                              // (no overlap: cut = N, nothing is faded, nothing is carried)
    if (N > cut) if (const int rc = hann_table(N - cut, &hann)) return rc;
#define GO(K, L) hipLaunchKernelGGL((k_clips_carry<K, L>), grid, blk, 0, s, frames, clip_frame0, (long long)n_clips, N, C, cut, prev_ptr, next_ptr, \
                                    hann, o, out_off, (long long)out_rows, be, raw)
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

int frad_clips_frame_cut(const void* src, const int64_t* row_src, const int32_t* row_valid, int64_t n_rows, int32_t row_len, int32_t step,
                         void* out, void* stream) {
    if (step < 1 || row_len < 1 || n_rows < 0) return FRAD_E_INVALID;
    if (n_rows == 0) return FRAD_OK;
    const long long rb = (long long)row_len * step;
    if (!src || !row_src || !row_valid || !out || n_rows > (0x7fffffffffffffffLL - 32) / rb) return FRAD_E_INVALID;
    const long long chunks = (n_rows * rb + 30) / 16, per_block = 256LL * CUT_K;       // (an upper bound: head <= 15)
    long long blocks = (chunks + per_block - 1) / per_block;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_clips_cut, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned char*>(src), row_src, row_valid, (long long)n_rows, rb, (int)step,
                       static_cast<unsigned char*>(out));
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

int frad_clips_carry_cut(const void* const* carry_ptr, const int32_t* carry_len, const void* src, const int64_t* src_off,
                         int64_t n_clips, const int32_t* row_clip, const int64_t* row_at, int64_t n_rows, int32_t row_len,
                         int32_t step, void* out, const int64_t* next_at, void* const* next_ptr, void* stream) {
    if (step < 1 || row_len < 1 || n_clips < 0 || n_rows < 0) return FRAD_E_INVALID;
    if (n_clips == 0) return FRAD_OK;
    const long long rb = (long long)row_len * step;
    if (!carry_ptr || !carry_len || !src || !src_off || (next_ptr && !next_at)) return FRAD_E_INVALID;
    if (n_rows > 0 && (!row_clip || !row_at || !out || n_rows > (0x7fffffffffffffffLL - 32) / rb)) return FRAD_E_INVALID;
    if (n_rows == 0 && !next_ptr) return FRAD_OK;              // no row and no remainder: nothing to write
    const long long chunks = n_rows ? (n_rows * rb + 30) / 16 : 0, per_block = 256LL * CUT_K;      // (an upper bound: head <= 15)
    long long blocks = (chunks + per_block - 1) / per_block;
    const long long for_clips = next_ptr ? (n_clips < 4096 ? n_clips : 4096) : 0;                  // a block per remainder
    if (blocks < for_clips) blocks = for_clips;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_clips_carry_cut, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned char* const*>(carry_ptr), carry_len, static_cast<const unsigned char*>(src), src_off,
                       (long long)n_clips, row_clip, row_at, (long long)n_rows, rb, (int)step, static_cast<unsigned char*>(out), next_at,
                       reinterpret_cast<unsigned char* const*>(next_ptr));
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

// ---- native frame-header scan (host code, no device involved) --------------------------------------------------------
static inline uint32_t be32(const unsigned char* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

int64_t frad_asfh_scan(const void* stream_bytes, int64_t nbytes, int64_t start, frad_frame_info* frames, int64_t max_frames,
                       int64_t* next_pos, int32_t* stop_reason) {
    static const unsigned char SIGN[4] = {0xff, 0xd0, 0xd2, 0x98};                     // common.py FRM_SIGN
    static const int SRATES[12] = {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000};
    if (!stream_bytes || nbytes < 0 || start < 0 || max_frames < 0 || (!frames && max_frames > 0) || !next_pos || !stop_reason) return FRAD_E_INVALID;
    const unsigned char* d = static_cast<const unsigned char*>(stream_bytes);
    int64_t pos = start, n = 0;
    *stop_reason = FRAD_SCAN_END;
    while (n < max_frames) {
        // next signature (decoder.py:82-90); keep the last three bytes when none is found: a signature may be split
        const unsigned char* at = nullptr;
        for (int64_t p = pos; p + 4 <= nbytes; ) {
            const void* hit = memchr(d + p, 0xff, (size_t)(nbytes - 3 - p));
            if (!hit) break;
            const unsigned char* h = static_cast<const unsigned char*>(hit);
            if (memcmp(h, SIGN, 4) == 0) { at = h; break; }
            p = (h - d) + 1;
        }
        if (!at) { pos = nbytes - 3 > pos ? nbytes - 3 : pos; *stop_reason = FRAD_SCAN_END; break; }
        const int64_t h0 = at - d;
        frad_frame_info fi; memset(&fi, 0, sizeof fi);
        fi.header_off = h0;
        if (nbytes - h0 < 9) { pos = h0; *stop_reason = FRAD_SCAN_PARTIAL_HEADER; break; }
        uint64_t len = be32(d + h0 + 4);
        const unsigned pfb = d[h0 + 8];
        fi.profile = (int32_t)(pfb >> 5); fi.ecc = (pfb >> 4) & 1; fi.little_endian = (pfb >> 3) & 1; fi.depth_idx = pfb & 7;
        const bool compact_prof = fi.profile == 1 || fi.profile == 2;
        int64_t hlen = compact_prof ? 12 : 32;
        if (nbytes - h0 < hlen) { pos = h0; *stop_reason = FRAD_SCAN_PARTIAL_HEADER; break; }
        if (compact_prof) {
            const unsigned css = ((unsigned)d[h0 + 9] << 8) | d[h0 + 10];
            fi.channels = (int32_t)(css >> 10) + 1;
            const unsigned si = (css >> 6) & 0xF;
            fi.srate = si < 12 ? SRATES[si] : 0;
            const unsigned fidx = (css >> 1) & 0x1F;
            fi.fsize = (int32_t)((fidx & 3) == 0 ? 128 : (fidx & 3) == 1 ? 160 : (fidx & 3) == 2 ? 192 : 224) << (fidx >> 2);
            fi.force_flush = (int32_t)(css & 1);
            if (fi.force_flush) {
                fi.payload_off = h0 + hlen; fi.payload_bytes = 0;
                frames[n++] = fi; pos = h0 + hlen;
                if (n == max_frames) { *stop_reason = FRAD_SCAN_TABLE_FULL; break; }
                continue;
            }
            fi.overlap_ratio = d[h0 + 11] ? d[h0 + 11] + 1 : 0;
            if (fi.ecc) {
                hlen = 16;
                if (nbytes - h0 < hlen) { pos = h0; *stop_reason = FRAD_SCAN_PARTIAL_HEADER; break; }
                fi.ecc_dsize = d[h0 + 12]; fi.ecc_codesize = d[h0 + 13]; fi.crc = ((uint32_t)d[h0 + 14] << 8) | d[h0 + 15];
            }
        } else {
            fi.channels = (int32_t)d[h0 + 9] + 1; fi.ecc_dsize = d[h0 + 10]; fi.ecc_codesize = d[h0 + 11];
            fi.srate = (int32_t)be32(d + h0 + 12); fi.fsize = (int32_t)be32(d + h0 + 24); fi.crc = be32(d + h0 + 28);
        }
        if (len == 0xFFFFFFFFull) {                            // 64-bit length extension (asfh.py:128-132)
            if (nbytes - h0 < hlen + 8) { pos = h0; *stop_reason = FRAD_SCAN_PARTIAL_HEADER; break; }
            len = ((uint64_t)be32(d + h0 + hlen) << 32) | be32(d + h0 + hlen + 4);
            hlen += 8;
        }
        fi.payload_off = h0 + hlen; fi.payload_bytes = (int64_t)len;
        if ((uint64_t)(nbytes - fi.payload_off) < len) { pos = h0; *stop_reason = FRAD_SCAN_PARTIAL_PAYLOAD; break; }
        frames[n++] = fi;
        pos = fi.payload_off + (int64_t)len;
        if (n == max_frames) { *stop_reason = FRAD_SCAN_TABLE_FULL; break; }
    }
    *next_pos = pos;
    return n;
}

}  // extern "C"
