// frad_spectral.hip -- the spectral stage behind StreamIndex.decode(..., features=spec): frad_clips_spectrum.
//
//   k_clips_spectrum  short-time Fourier transform of many ragged float64 windows [rows, K] in one launch: framing, the
//                     analysis window, an LDS-resident float64 FFT, |X|^2 or |X|, an optional banded filterbank, an optional
//                     logarithm, float32 or float64 stores.  DESIGN.md section 4m, include/frad_hip.h.
//
// A team of Plan<LOG2M>::TEAM lanes owns one frame-channel.  The n_fft = 2M real values x[n] w[n] are packed into M complex
// points z[n] = x[2n] w[2n] + i x[2n+1] w[2n+1], transformed by fft_team<double, LOG2M, false>, and split:
//   A = Z[k] + conj(Z[M-k]),  B = Z[k] - conj(Z[M-k]),  T = W_{2M}^k B,
//   X[k] = (A.x + T.y, A.y - T.x) / 2,   X[M-k] = (A.x - T.y, -A.y - T.x) / 2,      k = 0 .. M/2   (Z[M] = Z[0]).
// The other way to feed a complex transform with real data -- two frame-channels as the real and the imaginary part of one
// n_fft-point transform -- makes a frame's rounding depend on its partner: the same frame would give other bits in another
// launch, and an all-zero frame next to a loud one would not come out as zero.  The packing keeps a frame's values a function of
// its own n_fft inputs and the tables, and it halves the LDS per frame-channel.
//
// Overlapping frames (hop < n_fft): every team gathers its own rows from global memory.  The teams of a block are consecutive
// frame-channels, so the rows that neighbours share are read within the same few hundred cycles and come from L1/L2; a block's
// span is not staged in LDS, which would cost a second LDS write and read per value in a kernel whose time is the float64
// butterflies and their LDS exchanges, not its loads.
#include "frad_launch.hpp"
#include "../../include/frad_hip.h"
#include <cmath>

namespace frad {
namespace {

struct SpArgs {
    const double* const* src_ptr; const int32_t* valid; const int64_t* frame_off;      // per clip (device memory)
    long long n_clips, out_frames;
    int K, hop, center, power, n_bands;
    const double* window;                                                              // n_fft weights
    const int32_t* band_lo; const int32_t* band_len; const int64_t* band_off; const double* band_w; long long n_weights;
    double log_scale, floor, floor_log;
};

// block = 256 lanes = 256 / TEAM teams, one frame-channel ("unit") each: unit u = global frame * K + channel, units in the
// order of the output, so a block's stores are one contiguous run.  No lane leaves early: the teams of more than one wave
// synchronise with the block's barrier, and a team without a unit transforms zeros that nobody stores.
template <int LOG2M, typename OUT>
__global__ void __launch_bounds__(256) k_clips_spectrum(SpArgs a, const cx<double>* __restrict__ tw, const cx<double>* __restrict__ tw2,
                                                        OUT* __restrict__ out) {
    constexpr int M = 1 << LOG2M, N = 2 * M, TEAM = Plan<LOG2M>::TEAM, SH = Plan<LOG2M>::SH, UPB = 256 / TEAM;
    constexpr int PP = (M / 2) / TEAM;                         // bin pairs (k, M - k) per lane; k = M/2 goes to lane 0 on top
    FRAD_DYN_SMEM(smem);
    const int cf = threadIdx.x / TEAM, t = threadIdx.x - cf * TEAM;
    cx<double>* buf = reinterpret_cast<cx<double>*>(smem) + (long long)cf * M;
    long long last = a.frame_off[a.n_clips];
    if (last > a.out_frames) last = a.out_frames;              // never beyond what the caller sized
    const long long u = (long long)blockIdx.x * UPB + cf;
    const long long fg = u / a.K;
    const int c = (int)(u - fg * a.K);
    const bool live = fg >= (long long)a.frame_off[0] && fg < last;

    // ---- gather: rows f * hop (- n_fft/2) ..., times the window; rows outside [0, valid) are +0.0
    {
        const double* src = nullptr;
        long long r0 = 0;
        int valid = 0;
        if (live) {
            long long lo = 0, hi = a.n_clips;                  // the last clip that starts at or before frame fg
            while (hi - lo > 1) {
                const long long mid = (lo + hi) >> 1;
                if ((long long)a.frame_off[mid] <= fg) lo = mid; else hi = mid;
            }
            src = a.src_ptr[lo]; valid = a.valid[lo];
            r0 = (fg - (long long)a.frame_off[lo]) * a.hop - (a.center ? M : 0);
        }
#pragma unroll 4
        for (int i = 0; i < N / TEAM; ++i) {
            const int n = t + i * TEAM;
            const long long r = r0 + n;
            double v = 0.0;
            if (r >= 0 && r < valid) {
                const double x = *FRAD_GCPTR(double, src + r * a.K + c);
                v = x * *FRAD_GCPTR(double, a.window + n);
            }
            real_slot<double, SH>(buf, n) = v;
        }
    }
    team_sync<TEAM>();
    fft_team<double, LOG2M, false>(buf, t, tw);

    // ---- split into the n_fft/2 + 1 bins of the real transform, |X|^2 or |X|
    double pa[PP + 1], pb[PP + 1];
#pragma unroll
    for (int i = 0; i <= PP; ++i) {
        const int k = (i < PP) ? t + i * TEAM : M / 2;
        if (i == PP && t != 0) continue;
        const cx<double> zk = buf[phys<double, SH>(k)], zm = buf[phys<double, SH>((M - k) & (M - 1))];
        const cx<double> A = {zk.x + zm.x, zk.y - zm.y}, B = {zk.x - zm.x, zk.y + zm.y};
        const cx<double> T = cmul(B, tw2[k]);
        const double xr = (A.x + T.y) * 0.5, xi = (A.y - T.x) * 0.5;
        const double yr = (A.x - T.y) * 0.5, yi = (-A.y - T.x) * 0.5;
        const double xr2 = xr * xr, xi2 = xi * xi, yr2 = yr * yr, yi2 = yi * yi;
        pa[i] = xr2 + xi2;
        pb[i] = yr2 + yi2;
        if (a.power == 1) { pa[i] = sqrt(pa[i]); pb[i] = sqrt(pb[i]); }
    }
    team_sync<TEAM>();
    double* P = reinterpret_cast<double*>(buf);                // bins 0 .. M, plain order
#pragma unroll
    for (int i = 0; i <= PP; ++i) {
        const int k = (i < PP) ? t + i * TEAM : M / 2;
        if (i == PP && t != 0) continue;
        P[k] = pa[i];
        if (k < M / 2) P[M - k] = pb[i];
    }
    team_sync<TEAM>();

    // ---- banded sums, logarithm, conversion: one frame-channel's bins are contiguous in out
    if (!live) return;
    const int n_out = a.n_bands > 0 ? a.n_bands : M + 1;
    OUT* const o = out + u * n_out;
    for (int m = t; m < n_out; m += TEAM) {
        double v;
        if (a.n_bands > 0) {
            int lo = a.band_lo[m], len = a.band_len[m];
            long long off = a.band_off[m];
            if (lo < 0 || off < 0) len = 0;                    // (the caller checks its tables; a bad one reads nothing)
            if ((long long)lo + len > M + 1) len = M + 1 - lo;
            if (off + len > a.n_weights) len = (int)(a.n_weights - off);
            double acc = 0.0;
            for (int i = 0; i < len; ++i) {
                const double p = *FRAD_GCPTR(double, a.band_w + off + i) * P[lo + i];
                acc = acc + p;
            }
            v = acc;
        } else {
            v = P[m];
        }
        if (a.log_scale != 0.0) v = (v <= a.floor) ? a.floor_log : a.log_scale * log(v);
        *FRAD_GPTR(OUT, o + m) = (OUT)v;
    }
}

template <int LOG2M, typename OUT>
int launch_spectrum(const SpArgs& a, OUT* out, hipStream_t s) {
    constexpr int M = 1 << LOG2M, UPB = 256 / Plan<LOG2M>::TEAM;
    Tables t1, t2;
    int rc = get_tables(LOG2M, false, t1);
    if (rc != FRAD_OK) return rc;
    rc = get_tables(LOG2M + 1, false, t2);                     // W_{2M}^k, k <= M/2, for the split
    if (rc != FRAD_OK) return rc;
    const long long units = a.out_frames * a.K, blocks = (units + UPB - 1) / UPB;
    if (blocks > 0x7fffffffLL) return FRAD_E_UNSUPPORTED;
    const size_t lds = (size_t)UPB * M * sizeof(cx<double>);
    allow_lds(k_clips_spectrum<LOG2M, OUT>, lds);
    hipLaunchKernelGGL((k_clips_spectrum<LOG2M, OUT>), dim3((unsigned)blocks), dim3(256), lds, s, a,
                       static_cast<const cx<double>*>(t1.tw), static_cast<const cx<double>*>(t2.tw), out);
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

template <typename OUT>
int launch_spectrum_any(int log2m, const SpArgs& a, void* out, hipStream_t s) {
    OUT* o = static_cast<OUT*>(out);
    switch (log2m) {
        case 6: return launch_spectrum<6, OUT>(a, o, s);
        case 7: return launch_spectrum<7, OUT>(a, o, s);
        case 8: return launch_spectrum<8, OUT>(a, o, s);
        case 9: return launch_spectrum<9, OUT>(a, o, s);
        case 10: return launch_spectrum<10, OUT>(a, o, s);
        case 11: return launch_spectrum<11, OUT>(a, o, s);
        default: return FRAD_E_INVALID;
    }
}

}  // namespace
}  // namespace frad

using namespace frad;

extern "C" {

int frad_clips_spectrum(const double* const* src_ptr, const int32_t* valid, int64_t n_clips, int32_t K, const int64_t* frame_off,
                        int64_t out_frames, int32_t n_fft, int32_t hop, int32_t center, const double* window, int32_t power,
                        int32_t n_bands, const int32_t* band_lo, const int32_t* band_len, const int64_t* band_off, const double* band_w,
                        int64_t n_weights, double log_scale, double floor, double floor_log, int32_t out_dtype, void* out, void* stream) {
    int log2n = -1;
    for (int l = 7; l <= 12; ++l) if (n_fft == (1 << l)) log2n = l;
    if (log2n < 0 || hop < 1 || K < 1 || n_clips < 0 || out_frames < 0 || (power != 1 && power != 2) || n_bands < 0 || n_weights < 0 ||
        (center != 0 && center != 1) || (out_dtype != FRAD_PCM_F32LE && out_dtype != FRAD_PCM_F64LE))
        return FRAD_E_INVALID;
    if (log_scale != 0.0 && !(std::isfinite(log_scale) && floor > 0.0 && std::isfinite(floor) && std::isfinite(floor_log))) return FRAD_E_INVALID;
    if (n_clips == 0 || out_frames == 0) return FRAD_OK;
    if (!src_ptr || !valid || !frame_off || !window || !out) return FRAD_E_INVALID;
    if (n_bands > 0 && (!band_lo || !band_len || !band_off || !band_w)) return FRAD_E_INVALID;
    if (out_frames > (1LL << 40) / K) return FRAD_E_UNSUPPORTED;
    const SpArgs a{src_ptr, valid, frame_off, (long long)n_clips, (long long)out_frames, (int)K, (int)hop, (int)center, (int)power,
                   (int)n_bands, window, band_lo, band_len, band_off, band_w, (long long)n_weights, log_scale, floor, floor_log};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return out_dtype == FRAD_PCM_F32LE ? launch_spectrum_any<float>(log2n - 1, a, out, s) : launch_spectrum_any<double>(log2n - 1, a, out, s);
}

}  // extern "C"
