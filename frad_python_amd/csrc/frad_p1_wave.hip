// profile 1 on the wave-autonomous kernels (frad_wave.hpp, MODE 1): K7 / K8 at N = 2048, one or two channels.
// Instantiation and launch policy; 1 = launched, 0 = not applicable (the caller falls back to the one-shot kernels).
#include "frad_wave.hpp"
#include "frad_launch.hpp"

namespace frad {

const void* wave_blob();
int wave_grid(long long units);
bool wave_off();
int wave_stagger_steps();

namespace {
bool p1_wave_off() { static const bool d = [] { const char* e = tune("FRAD_TUNE_NO_WAVE_P1"); return e && e[0] == '1'; }(); return d; }

template <int LG, int CC>
void go_p1_fwd(const void* blob, int grid, hipStream_t s, const unsigned char* pcm, int32_t* q, const Geom& g, const P1Wave& pw) {
    allow_lds(k_p1_fwd_wave<LG, CC>, kWaveLdsBytesP1);
    hipLaunchKernelGGL((k_p1_fwd_wave<LG, CC>), dim3(grid), dim3(64 * kWaveWaves), kWaveLdsBytesP1, s, pcm, q, static_cast<const cx<double>*>(blob), g, pw);
}
template <int CC>
void go_p1_fwd_lg(int lg, const void* blob, int grid, hipStream_t s, const unsigned char* pcm, int32_t* q, const Geom& g, const P1Wave& pw) {
    switch (lg) {
        case 1: go_p1_fwd<1, CC>(blob, grid, s, pcm, q, g, pw); break;
        case 2: go_p1_fwd<2, CC>(blob, grid, s, pcm, q, g, pw); break;
        default: go_p1_fwd<3, CC>(blob, grid, s, pcm, q, g, pw); break;
    }
}
}  // namespace

#if defined(FRAD_WAVE_STAMPS)
extern "C" int frad_debug_wave_stamps_p1(unsigned long long* out, int reset) {      // this translation unit's copy of the counters
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_stamps), sizeof(z)) != hipSuccess) return -1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_wave_stamps), z, sizeof(z)) != hipSuccess) return -1;
    return 0;
}
#endif

// The largest |X[k]| 2^(bits - 1) a frame of this PCM type can hold.  The reference's DCT-II is forward-normalised (an average
// of the samples times cosines), so |X[k]| <= max |pcm| after to_f64: 1 for normalised integers, 2^(w - 1) (signed) or 2^w
// (unsigned) for big-endian integers that FRAD_RAW_BE_INTS leaves unscaled.  0 = the host knows no bound: float PCM is not clipped.
static double p1_wave_peak(const Geom& g, double scale) {
    const int kind = g.dtype >> 3, lg = (g.dtype >> 1) & 3, be = g.dtype & 1;
    if (kind == 2) return 0.0;
    if (!(be && g.raw_be)) return scale;
    return ldexp(scale, (8 << lg) - (kind == 1 ? 1 : 0));
}

// What K7's float32 decisions can represent (frad_wave.hpp: k7_pow04, k7_band_code, k7_quantise), as a bound on the scaled
// coefficients |x| <= peak, and so on every band's RMS:
//   * k7_pow04 refines its float32 seed by Newton steps that multiply with a float32 reciprocal of y^5 ~ (mean square)^2 =
//     rms^4.  With rms <= peak <= 2^31 that is at most 2^124 and its reciprocal at least 2^-124: both normal float32 numbers.
//     From rms = 2^32 on, (float)y^5 is +inf, its reciprocal 0, the steps correct nothing and the threshold keeps the seed's
//     1e-6 -- enough to mis-round a bin within 1e-4 of a tie;
//   * k7_quantise's exact branch takes a float32 reciprocal of y^4 div^3 ~ |x|^3 <= 2^93: inside float32 a fortiori;
//   * k7_band_code decides exactly only inside its table of 256 code boundaries.  A band's threshold is at most
//     max(rms^0.8, floor <= 1) x loss, so peak^0.8 x loss below (e/2)^(255^0.75) ~ 3.1e8 keeps every code <= 255 and the float32
//     estimate (absolute error ~ 3e-4 there) below the 255.4 at which the table route ends.  At peak = 2^31 that is loss < 10.8.
// Anything louder -- profile-1 depths beyond 32 bit on normalised PCM, most unscaled big-endian integers (s16be from 24 bit on,
// every s32be / s64be), extreme loss levels -- goes to the one-shot kernel, whose float64 arithmetic has no such range.
static bool p1_wave_in_range(const Geom& g, const P1Wave& pw) {
    static const double kCodeLimit = pow(2.718281828459045 / 2, pow(255.0, 0.75));
    const double peak = p1_wave_peak(g, pw.scale);
    if (!(peak > 0.0) || !(peak <= 0x1p31)) return false;
    const double t = pow(peak, 0.8);
    return (t > 1.0 ? t : 1.0) * pw.loss < kCodeLimit;
}

// K7.  Needs whole frames (n_valid = N), 16-byte aligned PCM rows (ai), integer PCM of 2, 4 or 8 bytes whose scaled coefficients
// stay inside what the kernel's float32 decisions represent (p1_wave_in_range; float64 PCM has no bound, so it never does).
int launch_p1_fwd_wave(int lg, hipStream_t s, const unsigned char* pcm, int32_t* q, const Geom& g, const P1Wave& pw, int ai) {
    if (wave_off() || p1_wave_off() || g.N != 2048 || (g.C != 1 && g.C != 2) || !ai || g.n_valid != g.N || lg < 1) return 0;
    if ((g.dtype >> 3) == 2 && lg <= 2) return 0;              // f16 / f32 PCM: the reference's mixed-precision path (one-shot kernels)
    if (pw.edge[26] < g.N || !aligned16(q) || pw.tqh == nullptr) return 0;
    if (!p1_wave_in_range(g, pw)) return 0;
    // the tail's band-energy pass (wave_p1_tail): a run of 32 consecutive bins touches at most three bands and a band spans at
    // most kK7Slots runs -- true for every table rate up to 48 kHz at this frame length
    for (int b = 0; b < 26 && pw.edge[b] < g.N; ++b) {
        if (pw.edge[b + 1] <= pw.edge[b]) return 0;                       // (bands are non-empty up to the one that holds bin N - 1)
        const int last = (pw.edge[b + 1] < g.N ? pw.edge[b + 1] : g.N) - 1;
        if ((last >> 5) - (pw.edge[b] >> 5) + 1 > kK7Slots) return 0;
    }
    auto band_at = [&](int k) { int b = 0; while (b < 25 && pw.edge[b + 1] <= k) ++b; return b; };
    for (int r = 0; r < g.N / 32; ++r) if (band_at(32 * r + 31) - band_at(32 * r) > 2) return 0;
    const void* blob = wave_blob();
    if (blob == nullptr) return 0;
    Geom gg = g;
    gg.cg = wave_stagger_steps(); gg.fpb = 0; gg.bits = 32; gg.le = 1; gg.payload_stride = (long long)g.N * g.C * 4;
    gg.ovf_flag = nullptr; gg.ovf_limit = 0.0;
    const int grid = wave_grid(g.C == 2 ? g.n_frames : (g.n_frames + 1) / 2);
    if (g.C == 2) go_p1_fwd_lg<2>(lg, blob, grid, s, pcm, q, gg, pw);
    else go_p1_fwd_lg<1>(lg, blob, grid, s, pcm, q, gg, pw);
    return 1;
}

// K8
int launch_p1_inv_wave(hipStream_t s, const int32_t* q, double* out, const Geom& g, const P1Wave& pw) {
    if (wave_off() || p1_wave_off() || g.N != 2048 || (g.C != 1 && g.C != 2)) return 0;
    if (!aligned16(out) || (reinterpret_cast<uintptr_t>(q) & 3) || pw.edge[26] < g.N || pw.deq == nullptr) return 0;
    const void* blob = wave_blob();
    if (blob == nullptr) return 0;
    const int grid = wave_grid(g.C == 2 ? g.n_frames : (g.n_frames + 1) / 2);
    Geom gg = g;
    gg.cg = wave_stagger_steps(); gg.fpb = 0; gg.bits = 32; gg.le = 1; gg.payload_stride = (long long)g.N * g.C * 4;
    const unsigned char* qb = reinterpret_cast<const unsigned char*>(q);
    if (g.C == 2) {
        allow_lds(k_p1_inv_wave<2>, kWaveLdsBytesP1);
        hipLaunchKernelGGL(k_p1_inv_wave<2>, dim3(grid), dim3(64 * kWaveWaves), kWaveLdsBytesP1, s, qb, out, static_cast<const cx<double>*>(blob), gg, pw);
    } else {
        allow_lds(k_p1_inv_wave<1>, kWaveLdsBytesP1);
        hipLaunchKernelGGL(k_p1_inv_wave<1>, dim3(grid), dim3(64 * kWaveWaves), kWaveLdsBytesP1, s, qb, out, static_cast<const cx<double>*>(blob), gg, pw);
    }
    return 1;
}

}  // namespace frad
