// frad_p1.hpp -- profile 1 (psychoacoustic quantiser) kernels K7 / K8 for gfx950.
//
//   K7  k_p1_fwd / k_p1_fwd_direct   to_f64 + zero-pad + DCT-II + 27-band masking thresholds + per-bin
//                                    divide + power-law quantise -> int32 q[N, C], tq[27, C]
//                                    (fourier/profile1.py:15-40, tools/p1tools.py:15-44)
//   K8  k_p1_inv / k_p1_inv_direct   dequantise + threshold spreading + inverse DCT -> float64 [N, C]
//                                    (fourier/profile1.py:65-77)
//       k_p1_ola                     decoder cross-fade of consecutive frames (decoder.py:28-46)
// Float64 throughout, like the reference on integer / f64 PCM.  Exp-Golomb + deflate stay on the host.
#pragma once
#include "frad_kernels.hpp"
#include "frad_wave.hpp"
#include <math.h>

namespace frad {

constexpr int P1_BANDS = 27;

// per launch constants, built on the host (see frad_p1.hip)
struct P1Tables {
    const unsigned char* band_of;  // device table [N]: band j with start_j <= k < start_{j+1} (j <= 25), 255 = none
    int edge[P1_BANDS + 1];      // band edges in bins, NOT clipped (p1tools.py:15-16)
    double floor_[P1_BANDS];     // min(ATH(band centre), 1.0)            (p1tools.py:25-31)
    double scale;                // 2^(bits-1)                            (profile1.py:9-10)
    double loss;                 // max(|loss_level|, 0.125)              (profile1.py:20)
    int nb_used;                 // bands before the first empty one      (p1tools.py:22: break)
    int f32;                     // float32 / float16 PCM: the reference does not widen it (pcmformat.py:35), so its DCT
                                 // and band energies are float32 and only the divide + quantiser are float64
};

// band edges clipped to N, by value (profile 2's kernel copies them to LDS)
struct P1Edges { int edge[P1_BANDS + 1]; };

// frad_global.hip: profile 1 through HBM workspaces (frames wider than a CU's LDS at a non-power-of-two size)
int global_p1_analogue(const unsigned char* pcm, int32_t* q, int32_t* tq, const Geom& g, const P1Tables& tb, hipStream_t s);
int global_p1_digital(const int32_t* q, const int32_t* tq, double* out, const Geom& g, const P1Tables& tb, hipStream_t s);
// frad_p1.hip: the overlap-add's Hann ramp hanning_in_overlap(L) (backend/__init__.py:3) as the reference's host computes it,
// a device table of L float64 per (device, L).  FRAD_OK or a status
int hann_table(int L, const double** out);

__device__ __forceinline__ double wave_sum_f64(double v) {
    return u2d(wave_allreduce_u64(d2u(v), [](u64 a, u64 b) { return d2u(u2d(a) + u2d(b)); }));
}

// |x|^0.75 with sign (p1tools.py:43) and its inverse |x|^(1/0.75) (p1tools.py:44).  a^0.75 = sqrt(a) * sqrt(sqrt(a)):
// two correctly rounded square roots and one product (<= 1.5 ulp) instead of a generic pow -- the value is rounded
// to an integer right after, so only results within ~1e-16 of a half-integer could differ from pow's.
__device__ __forceinline__ double p1_quant(double x) {
    const double a = fabs(x), r = sqrt(a);
    return copysign(r * sqrt(r), x) * (a != 0.0);
}
// |x|^(4/3) = |x| * cbrt(|x|) (the reference raises to 1/0.75, whose double differs from 4/3 by 2^-54 relative: far
// below the 1e-9 the decode contract states)
__device__ __forceinline__ double p1_dequant(double x) { const double a = fabs(x); return copysign(a * cbrt(a), x) * (a != 0.0); }

// LDS scratch of the quantiser stages, after the transform buffers:
//   thres[cf][27] | step[cf][27] | floor[28] (doubles) | edge[32] (ints, clipped to N) | band_of[N] (bytes)
// The per-launch tables arrive as kernel arguments; p1_tables_to_lds copies them once per block so that the
// data-dependent lookups below are LDS reads (a by-value struct indexed at run time lives in scratch memory).
__host__ __device__ constexpr int p1_scratch_bytes(int cfs, int N) { return cfs * P1_BANDS * 16 + 28 * 8 + 32 * 4 + ((N + 15) / 16) * 16; }

struct P1Lds {
    double* thres; double* step; double* floor_; int* edge; unsigned char* band;
};
__device__ __forceinline__ P1Lds p1_lds(unsigned char* scratch, int cfs) {
    P1Lds l;
    l.thres = reinterpret_cast<double*>(scratch);
    l.step = l.thres + cfs * P1_BANDS;
    l.floor_ = l.step + cfs * P1_BANDS;
    l.edge = reinterpret_cast<int*>(l.floor_ + 28);
    l.band = reinterpret_cast<unsigned char*>(l.edge + 32);
    return l;
}
__device__ __forceinline__ void p1_tables_to_lds(unsigned char* scratch, int cfs, const P1Tables& tb, int N) {
    const P1Lds l = p1_lds(scratch, cfs);
    if (threadIdx.x <= P1_BANDS) l.edge[threadIdx.x] = tb.edge[threadIdx.x] < N ? tb.edge[threadIdx.x] : N;
    if (threadIdx.x < P1_BANDS) l.floor_[threadIdx.x] = tb.floor_[threadIdx.x];
    if ((N & 3) == 0) {
        for (int i = threadIdx.x; i < N / 4; i += blockDim.x)
            reinterpret_cast<uint32_t*>(l.band)[i] = reinterpret_cast<const uint32_t*>(tb.band_of)[i];
    } else {
        for (int i = threadIdx.x; i < N; i += blockDim.x) l.band[i] = tb.band_of[i];
    }
}

// linear ramp between consecutive band starts, endpoint excluded (np.linspace as mapping_from_opus uses it,
// p1tools.py:35-41): y = start_j + i * step_j with step_j = (thres[j+1] - thres[j]) / (bins in band j), computed once
// per band; bins beyond the last start map to 0.
__device__ __forceinline__ void p1_ramp_steps(const P1Lds& l, int cfs) {
    for (int i = threadIdx.x; i < cfs * P1_BANDS; i += blockDim.x) {
        const int j = i % P1_BANDS;
        double st = 0.0;
        if (j < P1_BANDS - 1) {
            const int num = l.edge[j + 1] - l.edge[j];
            if (num > 0) st = (l.thres[i + 1] - l.thres[i]) / (double)num;
        }
        l.step[i] = st;
    }
}
// bin i of a band of `num` bins from t0 towards t1, st = (t1 - t0) / num
__device__ __forceinline__ double p1_ramp(double i, int num, double st, double t0, double t1) {
    double y = i * st;
    if (st == 0.0) y = (i / (double)num) * (t1 - t0);                                 // numpy's denormal-safe branch
    return y + t0;
}
__device__ __forceinline__ double p1_spread(const P1Lds& l, int cf, int k) {
    const int j = l.band[k];
    if (j >= P1_BANDS - 1) return 0.0;
    const double* thres = l.thres + cf * P1_BANDS;
    const int a = l.edge[j];
    return p1_ramp((double)(k - a), l.edge[j + 1] - a, l.step[cf * P1_BANDS + j], thres[j], thres[j + 1]);
}

// K7 epilogue: X[k] of `nfl` frames x `cw` channels sit in LDS (xslot<double, SH>); the channels are c0 .. c0+cw-1 of
// the frame's C (c0 = 0, cw = C unless the frame is transformed a channel group at a time); scratch as above for `cfs` slots.
template <int SH>
__device__ FRAD_NOINLINE void p1_quantise(int smem_off, int scratch_off, int slots, double scale, double loss, int nb_used, const Geom& g,
                                          long long f0, int nfl, int32_t* __restrict__ q, int32_t* __restrict__ tq,
                                          int c0, int cw, int cfs, int f32 = 0) {
    FRAD_DYN_SMEM(base);
    unsigned char* smem = base + smem_off;
    const int N = g.N, C = g.C, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const P1Lds l = p1_lds(base + scratch_off, cfs);
    // band energies: one (frame, channel, band) task per wave
    for (int task = wave; task < nfl * cw * P1_BANDS; task += nwaves) {
        const int b = task % P1_BANDS, cf = task / P1_BANDS;
        const int a = l.edge[b], e = l.edge[b + 1];
        double acc = 0.0;
        if (f32) for (int k = a + lane; k < e; k += 64) { const float v = (float)xslot<double, SH>(smem, cf, slots, k) * (float)scale; acc += (double)(v * v); }
        else for (int k = a + lane; k < e; k += 64) { const double v = xslot<double, SH>(smem, cf, slots, k) * scale; acc = fma(v, v, acc); }
        acc = wave_sum_f64(acc);
        if (lane == 0) l.thres[cf * P1_BANDS + b] = acc;
    }
    __syncthreads();
    // energies -> thresholds, one entry per thread (p1tools.py:18-33)
    for (int i = threadIdx.x; i < nfl * cw * P1_BANDS; i += blockDim.x) {
        const int b = i % P1_BANDS;
        double t = 0.0;
        if (b < nb_used) t = p1_band_threshold(l.thres[i], l.edge[b + 1] - l.edge[b], l.floor_[b], loss, f32);
        l.thres[i] = t;
    }
    __syncthreads();
    p1_ramp_steps(l, nfl * cw);
    // quantised thresholds, band-major / channel-minor
    for (int i = threadIdx.x; i < nfl * P1_BANDS * cw; i += blockDim.x) {
        const int fl = i / (P1_BANDS * cw), r = i - fl * P1_BANDS * cw, b = r / cw, j = r - b * cw;
        const double t = l.thres[(fl * cw + j) * P1_BANDS + b];
        const double v = log(t > 1.0 ? t : 1.0) / log(2.718281828459045 / 2);
        tq[(f0 + fl) * (long long)(P1_BANDS * C) + b * C + c0 + j] = (int32_t)rint(copysign(pow(fabs(v), 1.0 / 0.75), v));
    }
    __syncthreads();
    // per-bin divide + power-law quantiser, bin-major / channel-minor
    const int NW = N * cw;
    for (int i = threadIdx.x; i < nfl * NW; i += blockDim.x) {
        const int fl = i / NW, r = i - fl * NW, k = r / cw, j = r - k * cw, cf = fl * cw + j;
        double x = xslot<double, SH>(smem, cf, slots, k);
        if (f32) x = (double)(float)x;
        const double div = p1_spread(l, cf, k);
        q[(f0 + fl) * (long long)N * C + (long long)k * C + c0 + j] = p1w_quantise(x, div, scale);   // float32 where it decides, else exact
    }
}

// K8 prologue: q / tq -> X[k] in LDS (channels c0 .. c0+cw-1, as above).
template <int SH>
__device__ FRAD_NOINLINE void p1_dequantise(int smem_off, int scratch_off, int slots, double scale, const Geom& g,
                                            long long f0, int nfl, const int32_t* __restrict__ q, const int32_t* __restrict__ tq,
                                            int c0, int cw, int cfs) {
    FRAD_DYN_SMEM(base);
    unsigned char* smem = base + smem_off;
    const int N = g.N, C = g.C;
    const P1Lds l = p1_lds(base + scratch_off, cfs);
    for (int i = threadIdx.x; i < nfl * P1_BANDS * cw; i += blockDim.x) {
        const int fl = i / (P1_BANDS * cw), r = i - fl * P1_BANDS * cw, b = r / cw, j = r - b * cw;
        const double t = (double)tq[(f0 + fl) * (long long)(P1_BANDS * C) + b * C + c0 + j];
        l.thres[(fl * cw + j) * P1_BANDS + b] = pow(2.718281828459045 / 2, p1_quant(t));
    }
    __syncthreads();                                         // also orders p1_tables_to_lds (kernel start) before its readers
    p1_ramp_steps(l, nfl * cw);
    __syncthreads();
    const int NW = N * cw;
    for (int i = threadIdx.x; i < nfl * NW; i += blockDim.x) {
        const int fl = i / NW, r = i - fl * NW, k = r / cw, j = r - k * cw, cf = fl * cw + j;
        const double v = p1_dequant((double)q[(f0 + fl) * (long long)N * C + (long long)k * C + c0 + j]) / scale;
        xslot<double, SH>(smem, cf, slots, k) = v * p1_spread(l, cf, k);
    }
}

template <int LOG2M, int LG, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT <= 256 ? 2 : 1))
k_p1_fwd(const unsigned char* __restrict__ pcm, int32_t* __restrict__ q, int32_t* __restrict__ tq,
         const cx<double>* __restrict__ tw, const cx<double>* __restrict__ post, Geom g, P1Tables tb, int aligned_in) {
    constexpr int M = 1 << LOG2M, TEAM = Plan<LOG2M>::TEAM, SLOTS = padded_slots(M), SH = Plan<LOG2M>::SH;
    FRAD_DYN_SMEM(smem);
    const long long f0 = (long long)blockIdx.x * g.fpb;
    const long long rem = g.n_frames - f0;
    const int nfl = rem < g.fpb ? (int)rem : g.fpb;
    const int cf = threadIdx.x / TEAM, t = threadIdx.x - cf * TEAM;
    cx<double>* buf = reinterpret_cast<cx<double>*>(smem) + (long long)cf * SLOTS;
    p1_tables_to_lds(smem + g.fpb * g.C * SLOTS * 16, g.fpb * g.C, tb, g.N);
    stage_in_pcm<double, LG, SH, true>(pcm, 0, g, f0, nfl, SLOTS, aligned_in != 0);
    __syncthreads();
    fft_team<double, LOG2M, false>(buf, t, tw);
    dct_post<double, LOG2M>(buf, t, post);
    __syncthreads();
    p1_quantise<SH>(0, g.fpb * g.C * SLOTS * 16, SLOTS, tb.scale, tb.loss, tb.nb_used, g, f0, nfl, q, tq, 0, g.C, g.fpb * g.C, tb.f32);
}

template <int LOG2M, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT <= 256 ? 2 : 1))
k_p1_inv(const int32_t* __restrict__ q, const int32_t* __restrict__ tq, double* __restrict__ out,
         const cx<double>* __restrict__ tw, const cx<double>* __restrict__ post, Geom g, P1Tables tb) {
    constexpr int M = 1 << LOG2M, TEAM = Plan<LOG2M>::TEAM, SLOTS = padded_slots(M), SH = Plan<LOG2M>::SH;
    FRAD_DYN_SMEM(smem);
    const long long f0 = (long long)blockIdx.x * g.fpb;
    const long long rem = g.n_frames - f0;
    const int nfl = rem < g.fpb ? (int)rem : g.fpb;
    const int cf = threadIdx.x / TEAM, t = threadIdx.x - cf * TEAM;
    cx<double>* buf = reinterpret_cast<cx<double>*>(smem) + (long long)cf * SLOTS;
    p1_tables_to_lds(smem + g.fpb * g.C * SLOTS * 16, g.fpb * g.C, tb, g.N);
    p1_dequantise<SH>(0, g.fpb * g.C * SLOTS * 16, SLOTS, tb.scale, g, f0, nfl, q, tq, 0, g.C, g.fpb * g.C);
    __syncthreads();
    dct_pre_inverse<double, LOG2M>(buf, t, post);
    fft_team<double, LOG2M, true>(buf, t, tw);
    __syncthreads();
    store_pcm_f64<SH, true>(0, out, g, f0, nfl, SLOTS);
}

// The frames the table-driven wave kernel (k_p1_inv_wave) marked: redo[0] = count, redo[1 + i] = frame index.  One frame per
// block pass (launch with g.fpb = 1), the exact arithmetic of k_p1_inv; runs behind the wave kernel on the same stream and
// overwrites its output for those frames.
template <int LOG2M, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT <= 256 ? 2 : 1))
k_p1_inv_redo(const int32_t* __restrict__ q, const int32_t* __restrict__ tq, double* __restrict__ out,
              const cx<double>* __restrict__ tw, const cx<double>* __restrict__ post, Geom g, P1Tables tb, const int* __restrict__ redo) {
    constexpr int M = 1 << LOG2M, TEAM = Plan<LOG2M>::TEAM, SLOTS = padded_slots(M), SH = Plan<LOG2M>::SH;
    FRAD_DYN_SMEM(smem);
    const int count = redo[0];
    if ((int)blockIdx.x >= count) return;
    const int cf = threadIdx.x / TEAM, t = threadIdx.x - cf * TEAM;
    cx<double>* buf = reinterpret_cast<cx<double>*>(smem) + (long long)cf * SLOTS;
    p1_tables_to_lds(smem + g.C * SLOTS * 16, g.C, tb, g.N);
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        const long long f0 = redo[1 + i];
        p1_dequantise<SH>(0, g.C * SLOTS * 16, SLOTS, tb.scale, g, f0, 1, q, tq, 0, g.C, g.C);
        __syncthreads();
        int tt = t; FRAD_OPAQUE(tt);
        dct_pre_inverse<double, LOG2M>(buf, tt, post);
        fft_team<double, LOG2M, true>(buf, tt, tw);
        __syncthreads();
        store_pcm_f64<SH, true>(0, out, g, f0, 1, SLOTS);
        __syncthreads();
    }
}

// Frames whose channels exceed a CU's LDS: one frame per block, g.cg channels per pass (stage / transform / quantise
// per group; the quantiser works channel by channel, so groups are independent).
template <int LOG2M, int LG, int MAXT>
__global__ void __launch_bounds__(MAXT)
k_p1_fwd_grp(const unsigned char* __restrict__ pcm, int32_t* __restrict__ q, int32_t* __restrict__ tq,
             const cx<double>* __restrict__ tw, const cx<double>* __restrict__ post, Geom g, P1Tables tb) {
    constexpr int M = 1 << LOG2M, TEAM = Plan<LOG2M>::TEAM, SLOTS = padded_slots(M), SH = Plan<LOG2M>::SH;
    FRAD_DYN_SMEM(smem);
    const long long f0 = blockIdx.x;
    const int cf = threadIdx.x / TEAM, t = threadIdx.x - cf * TEAM, cg = g.cg;
    cx<double>* buf = reinterpret_cast<cx<double>*>(smem) + (long long)cf * SLOTS;
    const int scratch_off = cg * SLOTS * 16;
    p1_tables_to_lds(smem + scratch_off, cg, tb, g.N);
    for (int c0 = 0; c0 < g.C; c0 += cg) {
        const int cgn = g.C - c0 < cg ? g.C - c0 : cg;
        stage_in_pcm_group<double, LG, SH>(pcm, 0, g, f0, SLOTS, c0, cgn);
        __syncthreads();
        int tt = t; FRAD_OPAQUE(tt);
        fft_team<double, LOG2M, false>(buf, tt, tw);
        dct_post<double, LOG2M>(buf, tt, post);
        __syncthreads();
        p1_quantise<SH>(0, scratch_off, SLOTS, tb.scale, tb.loss, tb.nb_used, g, f0, 1, q, tq, c0, cgn, cg, tb.f32);
        __syncthreads();
    }
}

template <int LOG2M, int MAXT>
__global__ void __launch_bounds__(MAXT)
k_p1_inv_grp(const int32_t* __restrict__ q, const int32_t* __restrict__ tq, double* __restrict__ out,
             const cx<double>* __restrict__ tw, const cx<double>* __restrict__ post, Geom g, P1Tables tb) {
    constexpr int M = 1 << LOG2M, TEAM = Plan<LOG2M>::TEAM, SLOTS = padded_slots(M), SH = Plan<LOG2M>::SH;
    FRAD_DYN_SMEM(smem);
    const long long f0 = blockIdx.x;
    const int cf = threadIdx.x / TEAM, t = threadIdx.x - cf * TEAM, cg = g.cg;
    cx<double>* buf = reinterpret_cast<cx<double>*>(smem) + (long long)cf * SLOTS;
    const int scratch_off = cg * SLOTS * 16;
    p1_tables_to_lds(smem + scratch_off, cg, tb, g.N);
    for (int c0 = 0; c0 < g.C; c0 += cg) {
        const int cgn = g.C - c0 < cg ? g.C - c0 : cg;
        p1_dequantise<SH>(0, scratch_off, SLOTS, tb.scale, g, f0, 1, q, tq, c0, cgn, cg);
        __syncthreads();
        int tt = t; FRAD_OPAQUE(tt);
        dct_pre_inverse<double, LOG2M>(buf, tt, post);
        fft_team<double, LOG2M, true>(buf, tt, tw);
        __syncthreads();
        store_pcm_group<SH>(0, out, g, f0, SLOTS, c0, cgn);
        __syncthreads();
    }
}

// any legal compact frame size (160/192/224 * 2^n ...): direct cosine sums, one frame per block
template <int LG>
__global__ void __launch_bounds__(256) k_p1_fwd_direct(const unsigned char* __restrict__ pcm, int32_t* __restrict__ q, int32_t* __restrict__ tq,
                                                       const double* __restrict__ ct, Geom g, P1Tables tb, int aligned_in) {
    FRAD_DYN_SMEM(smem);
    const int N = g.N, C = g.C;
    const long long f0 = blockIdx.x;
    double* x = reinterpret_cast<double*>(smem);
    double* X = x + (long long)N * C;
    p1_tables_to_lds(smem + 2 * N * C * 8, C, tb, N);
    stage_in_pcm<double, LG, -1, false>(pcm, 0, g, f0, 1, N, aligned_in != 0);
    __syncthreads();
    const double inv_n = 1.0 / (double)N;
    const unsigned fourN = 4u * (unsigned)N;
    for (int i = threadIdx.x; i < N * C; i += blockDim.x) {
        const int c = i / N, k = i - c * N;
        const double* xc = x + (long long)c * N;
        double acc = 0.0;
        unsigned j = (unsigned)k % fourN;
        const unsigned step = (2u * (unsigned)k) % fourN;
        for (int n = 0; n < N; ++n) { acc = fma(xc[n], ct[j], acc); j += step; if (j >= fourN) j -= fourN; }
        X[(long long)c * N + k] = acc * inv_n;
    }
    __syncthreads();
    p1_quantise<-1>(N * C * 8, 2 * N * C * 8, N, tb.scale, tb.loss, tb.nb_used, g, f0, 1, q, tq, 0, C, C, tb.f32);
}

template <int UNUSED>
__global__ void __launch_bounds__(256) k_p1_inv_direct(const int32_t* __restrict__ q, const int32_t* __restrict__ tq, double* __restrict__ out,
                                                       const double* __restrict__ ct, Geom g, P1Tables tb) {
    FRAD_DYN_SMEM(smem);
    const int N = g.N, C = g.C;
    const long long f0 = blockIdx.x;
    double* X = reinterpret_cast<double*>(smem);
    double* x = X + (long long)N * C;
    p1_tables_to_lds(smem + 2 * N * C * 8, C, tb, N);
    p1_dequantise<-1>(0, 2 * N * C * 8, N, tb.scale, g, f0, 1, q, tq, 0, C, C);
    __syncthreads();
    const unsigned fourN = 4u * (unsigned)N;
    for (int i = threadIdx.x; i < N * C; i += blockDim.x) {
        const int c = i / N, n = i - c * N;
        const double* Xc = X + (long long)c * N;
        double acc = 0.0;
        const unsigned step = (2u * (unsigned)n + 1u) % fourN;
        unsigned j = step;
        for (int k = 1; k < N; ++k) { acc = fma(Xc[k], ct[j], acc); j += step; if (j >= fourN) j -= fourN; }
        x[(long long)c * N + n] = Xc[0] + 2.0 * acc;
    }
    __syncthreads();
    store_pcm_f64<-1, false>(N * C * 8, out, g, f0, 1, N);
}

// profile 2 (fourier/profile2.py:69-86, tools/p2tools.py:105-115): dequantise, TNS synthesis, threshold ramp -> the
// coefficient plane [n_frames, N, C] (float64), which frad_p0_digital then inverts as a 64-bit little-endian payload.
// The synthesis filter 1 / A(z) runs along the bins, a serial recursion per (frame, channel): one lane per channel, 64
// consecutive (frame, channel) pairs per wave, all lanes at the same bin (the band changes are uniform).  The state is
// direct form II transposed in scipy.signal.lfilter's order (y = z0 + x; z_k = z_{k+1} - a_{k+1} y; b = [1]), so every
// rounding is the reference's.  The fallback (a NaN, an Inf or |y| > 1e6 anywhere in the channel -> the unfiltered
// coefficients) is decided as the filter runs; the rare channel that trips it is rewritten in a second pass.  N is a
// multiple of 32 (compact sizes), so every lane reads its bins P2_CHUNK at a time, those loads in flight together (staging the
// chunks through LDS for coalesced rows was measured slower: DESIGN.md section 4d).
constexpr int P2_ORDER = 12;
constexpr int P2_CHUNK = 16;
__device__ __forceinline__ double p2_thres(const int32_t* __restrict__ tq, long long row, int C, int b) {
    return pow(2.718281828459045 / 2, p1_quant((double)tq[row + (long long)b * C]));
}
template <int UNUSED>
__global__ void __launch_bounds__(64) k_p2_synth(const int32_t* __restrict__ q, const int32_t* __restrict__ tq, const int32_t* __restrict__ lpc,
                                                 double* __restrict__ out, long long n_frames, int N, int C, double scale,
                                                 const unsigned char* __restrict__ band_of, P1Edges pe) {
    FRAD_DYN_SMEM(smem);
    unsigned char* band = smem;
    int* edge = reinterpret_cast<int*>(smem + ((N + 15) / 16) * 16);
    for (int i = threadIdx.x; i < N / 4; i += blockDim.x) reinterpret_cast<uint32_t*>(band)[i] = reinterpret_cast<const uint32_t*>(band_of)[i];
    if (threadIdx.x <= P1_BANDS) edge[threadIdx.x] = pe.edge[threadIdx.x];
    __syncthreads();
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= n_frames * C) return;
    const long long f = g / C;
    const int c = (int)(g - f * C);
    const int32_t* qc = q + f * (long long)N * C + c;
    double* oc = out + f * (long long)N * C + c;
    const long long trow = f * (long long)(P1_BANDS * C) + c;
    double a[P2_ORDER];
    bool filt = false;
    {
        const int32_t* lc = lpc + f * (long long)((P2_ORDER + 1) * C) + c;
        filt = lc[0] != 0;                                   // index 0 only decides "all zero" (dequantise_lpc)
#pragma unroll
        for (int i = 0; i < P2_ORDER; ++i) { const int32_t v = lc[(long long)(i + 1) * C]; filt |= v != 0; a[i] = (double)v / 15.0; }
    }
    for (int pass = 0; pass < 2; ++pass) {
        double z[P2_ORDER];
#pragma unroll
        for (int i = 0; i < P2_ORDER; ++i) z[i] = 0.0;
        bool bad = false;
        int cj = -1, ca = 0, cnum = 1;
        double t0 = 0.0, t1 = 0.0, st = 0.0;
        for (int k0 = 0; k0 < N; k0 += P2_CHUNK) {
            int32_t qv[P2_CHUNK];
#pragma unroll
            for (int u = 0; u < P2_CHUNK; ++u) qv[u] = qc[(long long)(k0 + u) * C];
#pragma unroll
            for (int u = 0; u < P2_CHUNK; ++u) {
                const int k = k0 + u;
                const double x = p1_dequant((double)qv[u]) / scale;
                double y = x;
                if (filt) {
                    y = z[0] + x;
#pragma unroll
                    for (int i = 0; i < P2_ORDER - 1; ++i) z[i] = z[i + 1] - y * a[i];
                    z[P2_ORDER - 1] = 0.0 - y * a[P2_ORDER - 1];
                    bad |= !(fabs(y) <= 1e6);
                }
                const int j = band[k];                       // the same bin in every lane: uniform
                if (j != cj) {
                    cj = j;
                    if (j < P1_BANDS - 1) {
                        ca = edge[j]; cnum = edge[j + 1] - ca;
                        t0 = p2_thres(tq, trow, C, j); t1 = p2_thres(tq, trow, C, j + 1);
                        st = cnum > 0 ? (t1 - t0) / (double)cnum : 0.0;
                    }
                }
                const double r = j < P1_BANDS - 1 ? p1_ramp((double)(k - ca), cnum, st, t0, t1) : 0.0;
                oc[(long long)k * C] = y * r;
            }
        }
        if (!(filt && bad)) break;
        filt = false;                                        // the fallback: the same channel, unfiltered
    }
}

// profile 2 analysis (fourier/profile2.py:15-55, tools/p2tools.py:55-103): per (frame, channel) the 27 masking thresholds
// and the divisor ramp of profile 1, the masked spectrum m = X / div, then tns_analysis -- the order-12 LPC of m and, when
// it predicts well, the FIR residual in its place -- and the power-law quantiser.  One block per (frame, channel) over the
// float64 DCT plane [n_frames, N, C] that frad_p0_analogue wrote (norm='forward'); m overwrites X in place (each block owns
// its column), and every later pass reads it back through L2: a channel's spectrum at N = 28 672 is 224 KiB, more than a
// CU's LDS, so one code path serves all 32 compact sizes.  Reductions are block sums (wave sums, then the wave partials in
// order), not numpy's pairwise order: they decide only comparisons and the LPC's rounding.  The
// Levinson-Durbin recursion runs on one lane, in float64, with the reference's 0.96 clamp and early exits.  The residual is
// np.convolve's (scipy.signal.lfilter routes a FIR filter there): on the reference platform a sequential fused multiply-add
// from the oldest tap, r[k] = fma(b12, m[k-12], ... fma(b1, m[k-1], 0)) + m[k] -- reproduced here bit for bit.
constexpr int P2_THREADS = 256;
constexpr int P2_RED = (P2_ORDER + 1) * (P2_THREADS / 64 + 1);             // doubles of the block-sum scratch

// block sums of P values per thread; every thread gets the totals.  red: P2_RED doubles of LDS
template <int P>
__device__ __forceinline__ void p2_block_sum(double (&v)[P], double* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
#pragma unroll
    for (int p = 0; p < P; ++p) { const double s = wave_sum_f64(v[p]); if (lane == 0) red[wave * P + p] = s; }
    __syncthreads();
    if (threadIdx.x < P) { double s = 0.0; for (int w = 0; w < nw; ++w) s += red[w * P + threadIdx.x]; red[nw * P + threadIdx.x] = s; }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < P; ++p) v[p] = red[nw * P + p];
    __syncthreads();
}
__device__ __forceinline__ double p2_block_max(double v, double* red) {            // v >= 0 (or NaN, which fmax drops)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    v = u2d(wave_allreduce_u64(d2u(v), [](u64 a, u64 b) { return d2u(fmax(u2d(a), u2d(b))); }));
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < nw; ++w) r = fmax(r, red[w]);
    __syncthreads();
    return r;
}
// numpy's sum of n <= 12 float64 values (pairwise_sum below its block size: a plain loop under 8 values, else 8 partial
// sums combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and the rest added in order)
__device__ __forceinline__ double p2_np_sum(const double* a, int n) {
    if (n < 8) { double s = 0.0; for (int i = 0; i < n; ++i) s += a[i]; return s; }
    double s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    for (int i = 8; i < n; ++i) s += a[i];
    return s;
}
// levinson_durbin + quantise_lpc (p2tools.py:17-50): r[0..12] -> lq[0..12] (lq[0] = 0); false = tns_analysis gives up here
__device__ __forceinline__ bool p2_levinson(const double* r, int* lq) {
    double lpc[P2_ORDER + 1], tmp[P2_ORDER + 1], prod[P2_ORDER];
    lpc[0] = 1.0;
    for (int i = 1; i <= P2_ORDER; ++i) lpc[i] = 0.0;
    double err = r[0];
    if (err > 1e-10) {
        for (int i = 1; i <= P2_ORDER; ++i) {
            for (int j = 0; j < i; ++j) prod[j] = lpc[j] * r[i - j];
            double refl = -p2_np_sum(prod, i) / err;
            if (fabs(refl) >= 0.96) refl = refl > 0 ? 0.96 : -0.96;        // 0.96 * np.sign (NaN cannot reach here)
            for (int j = 0; j <= P2_ORDER; ++j) tmp[j] = lpc[j];
            lpc[i] = refl;
            for (int j = 1; j < i; ++j) lpc[j] += refl * tmp[i - j];
            err *= 1.0 - refl * refl;
            if (err <= 1e-12) break;
        }
    }
    for (int j = 0; j < P2_ORDER; ++j) prod[j] = fabs(lpc[j + 1]);
    if (!(p2_np_sum(prod, P2_ORDER) >= 0.01)) return false;               // np.sum(np.abs(lpc[1:])) < 0.01
    bool any = false;
    lq[0] = 0;
    for (int j = 1; j <= P2_ORDER; ++j) {
        double v = lpc[j] * 15.0;
        v = v < -15.0 ? -15.0 : (v > 14.0 ? 14.0 : v);                    // np.clip, then round half to even
        lq[j] = (int)rint(v);
        any |= lq[j] != 0;
    }
    return any;
}
// the FIR residual at bin k of the masked column m (stride C); b[1..12] = lq / 15
__device__ __forceinline__ double p2_residual(const double* __restrict__ m, int C, int k, const double* b) {
    double acc = 0.0;
    const int i0 = k < P2_ORDER ? k : P2_ORDER;
    for (int i = i0; i >= 1; --i) acc = fma(b[i], m[(long long)(k - i) * C], acc);
    return m[(long long)k * C] + acc;
}

template <int UNUSED>
__global__ void __launch_bounds__(P2_THREADS) k_p2_analysis(double* __restrict__ X, int32_t* __restrict__ q, int32_t* __restrict__ tq,
                                                            int32_t* __restrict__ lpc, long long n_frames, int N, int C, P1Tables tb) {
    FRAD_DYN_SMEM(smem);
    double* red = reinterpret_cast<double*>(smem);                       // P2_RED doubles
    double* bco = red + P2_RED;                                          // b[0..12] of the FIR; bco[13] = use-TNS flag
    int* lqs = reinterpret_cast<int*>(bco + 16);                         // the 13 LPC integers
    unsigned char* scratch = reinterpret_cast<unsigned char*>(lqs + 16);  // P1Lds for one channel
    const long long g = blockIdx.x;
    const long long f = g / C;
    const int c = (int)(g - f * C), wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    double* x = X + f * (long long)N * C + c;
    const P1Lds l = p1_lds(scratch, 1);
    p1_tables_to_lds(scratch, 1, tb, N);
    __syncthreads();
    // band energies of X * 2^(bits-1) and the thresholds, as profile 1's quantiser (p1_quantise)
    for (int b = wave; b < P1_BANDS; b += nw) {
        const int a = l.edge[b], e = l.edge[b + 1];
        double acc = 0.0;
        if (tb.f32) for (int k = a + lane; k < e; k += 64) { const float v = (float)x[(long long)k * C] * (float)tb.scale; acc += (double)(v * v); }
        else for (int k = a + lane; k < e; k += 64) { const double v = x[(long long)k * C] * tb.scale; acc = fma(v, v, acc); }
        acc = wave_sum_f64(acc);
        if (lane == 0) l.thres[b] = acc;
    }
    __syncthreads();
    if (threadIdx.x < P1_BANDS) {
        const int b = threadIdx.x;
        l.thres[b] = b < tb.nb_used ? p1_band_threshold(l.thres[b], l.edge[b + 1] - l.edge[b], l.floor_[b], tb.loss, tb.f32) : 0.0;
    }
    __syncthreads();
    p1_ramp_steps(l, 1);
    if (threadIdx.x < P1_BANDS) {
        const int b = threadIdx.x;
        const double t = l.thres[b];
        const double v = log(t > 1.0 ? t : 1.0) / log(2.718281828459045 / 2);
        tq[f * (long long)(P1_BANDS * C) + b * C + c] = (int32_t)rint(copysign(pow(fabs(v), 1.0 / 0.75), v));
    }
    __syncthreads();
    // m = X / div in place (div 0 = inf, profile2.py:31); the statistics of lpc_cond and the energy test on the way
    double s1[4] = {0.0, 0.0, 0.0, 0.0};                                 // sum m, sum |m|, sum log(|m| + 1e-10), sum m^2
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        double v = x[(long long)k * C];
        if (tb.f32) v = (double)(float)v;
        const double div = p1_spread(l, 0, k);
        v = v / (div == 0.0 ? (double)INFINITY : div);
        x[(long long)k * C] = v;
        s1[0] += v; s1[1] += fabs(v); s1[2] += log(fabs(v) + 1e-10); s1[3] = fma(v, v, s1[3]);
    }
    p2_block_sum<4>(s1, red);                                            // (its barriers also publish m to the block)
    const double dn = (double)N;
    const double mean = s1[0] / dn;
    bool tns = N >= 2 * P2_ORDER && exp(s1[2] / dn) / (s1[1] / dn + 1e-10) < 0.5 && !(s1[3] < 1e-10);
    double oe = 0.0;                                                     // sum (m - mean)^2: calc_autocorr's norm and predgain's
    if (tns) {
        double s2[1] = {0.0};
        for (int k = threadIdx.x; k < N; k += blockDim.x) { const double d = x[(long long)k * C] - mean; s2[0] = fma(d, d, s2[0]); }
        p2_block_sum<1>(s2, red);
        oe = s2[0];
        const double nrm = sqrt(oe), dv = nrm > 1e-6 ? nrm : 1.0;
        double r[P2_ORDER + 1];
#pragma unroll
        for (int i = 0; i <= P2_ORDER; ++i) r[i] = 0.0;
        for (int k = threadIdx.x; k < N; k += blockDim.x) {
            const double sk = (x[(long long)k * C] - mean) / dv;
#pragma unroll
            for (int i = 0; i <= P2_ORDER; ++i)
                if (k + i < N) r[i] = fma(sk, (x[(long long)(k + i) * C] - mean) / dv, r[i]);
        }
        p2_block_sum<P2_ORDER + 1>(r, red);
        if (threadIdx.x == 0) {
            for (int i = 0; i <= P2_ORDER; ++i) { const double w = (double)i * 0.01; r[i] *= exp(-0.5 * (w * w)); }
            const bool ok = p2_levinson(r, lqs);
            bco[0] = 1.0;
            for (int i = 1; i <= P2_ORDER; ++i) bco[i] = (double)lqs[i] / 15.0;
            bco[P2_ORDER + 1] = ok ? 1.0 : 0.0;
        }
        __syncthreads();
        tns = bco[P2_ORDER + 1] != 0.0;
    }
    if (tns) {                                                           // the residual: finite, <= 1e6, and a prediction gain
        double s3[2] = {0.0, 0.0};                                       // non-finite count, sum r
        double mx = 0.0;
        for (int k = threadIdx.x; k < N; k += blockDim.x) {
            const double rv = p2_residual(x, C, k, bco);
            s3[0] += isfinite(rv) ? 0.0 : 1.0;
            s3[1] += rv;
            mx = fmax(mx, fabs(rv));
        }
        p2_block_sum<2>(s3, red);
        mx = p2_block_max(mx, red);
        tns = s3[0] == 0.0 && mx <= 1e6;
        if (tns) {
            const double rmean = s3[1] / dn;
            double s4[1] = {0.0};
            for (int k = threadIdx.x; k < N; k += blockDim.x) { const double d = p2_residual(x, C, k, bco) - rmean; s4[0] = fma(d, d, s4[0]); }
            p2_block_sum<1>(s4, red);
            const double re = s4[0];
            const double gain = (oe < 1e-10 || re < 1e-10 || re >= oe) ? 0.0 : 20.0 * log10(oe / re);
            tns = gain >= 0.030102999566398120;                          // MIN_PRED = log10(2) / 10
        }
    }
    if (threadIdx.x <= P2_ORDER) lpc[f * (long long)((P2_ORDER + 1) * C) + (long long)threadIdx.x * C + c] = tns ? lqs[threadIdx.x] : 0;
    int32_t* qc = q + f * (long long)N * C + c;
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        const double v = tns ? p2_residual(x, C, k, bco) : x[(long long)k * C];
        qc[(long long)k * C] = p1w_quantise(v, 1.0, tb.scale);
    }
}
__host__ __device__ constexpr int p2_analysis_lds(int N) { return (P2_RED + 16) * 8 + 16 * 4 + p1_scratch_bytes(1, N); }

// R8: decoder overlap-add over a batch of consecutive frames (decoder.py:28-46).  Frame i keeps
// rows [0, cut) -- its first L = N - cut rows cross-faded with frame i-1's tail -- and hands its
// own tail [cut, N) to frame i+1.  out: [n_frames, cut, C]; next_tail: [L, C].
// element i of the overlap-added output [n_frames, cut, C] (decoder.py:31-38); win = hann_table(L): the weights are the
// host's, so that the cross-faded samples are the reference's bit for bit (the device's cos differs from the host's in the last
// bit for about one argument in 500)
__device__ __forceinline__ double p1_ola_value(const double* __restrict__ frames, const double* __restrict__ prev_tail,
                                               const double* __restrict__ win, int N, int C, int cut, long long i) {
    const int L = N - cut;
    const long long f = i / ((long long)cut * C);
    const int r = (int)(i - f * (long long)cut * C), n = r / C, c = r - n * C;
    double v = frames[(f * N + n) * C + c];
    if (n < L) {
        const double* tail = f > 0 ? frames + ((f - 1) * N + cut) * C : prev_tail;
        if (tail != nullptr) {
            const double w_in = win[n], w_out = win[L - 1 - n];       // fade_in[i], fade_in[olap_len - i - 1] (decoder.py:36-37)
            v = v * w_in;
            v = v + tail[(long long)n * C + c] * w_out;
        }
    }
    return v;
}

template <int UNUSED>
__global__ void __launch_bounds__(256) k_p1_ola(const double* __restrict__ frames, long long n_frames, int N, int C, int cut,
                                                const double* __restrict__ prev_tail, const double* __restrict__ win,
                                                double* __restrict__ out, double* __restrict__ next_tail) {
    const int L = N - cut;
    const long long total = n_frames * (long long)cut * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        out[i] = p1_ola_value(frames, prev_tail, win, N, C, cut, i);
    if (next_tail != nullptr && n_frames > 0)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)L * C; i += (long long)gridDim.x * blockDim.x)
            next_tail[i] = frames[((n_frames - 1) * N + cut) * C + i];
}

}  // namespace frad
