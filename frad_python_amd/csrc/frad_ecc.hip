// frad_ecc.hip -- Reed-Solomon frame protection and repair on the device (the reference's tools/ecc.py, which calls
// reedsolo.RSCodec(codesize, dsize + codesize) with the library defaults): GF(2^8) with primitive polynomial 0x11d,
// generator alpha = 2, first consecutive root 0, g(x) = prod_{i < codesize} (x - alpha^i), systematic blocks
// data || (data * x^codesize mod g).
//
// A batch is n frames back to back in one buffer (frame f at in_off[f] .. in_off[f+1]); every frame is cut into blocks
// (dsize data bytes on encode, dsize + codesize stored bytes on repair, the last block of a frame may be shorter) and
// the blocks of all frames are numbered globally (frame f owns blocks blk_off[f] .. blk_off[f+1]).
//
// k_rs_blocks: one lane per block, one wave per 64 consecutive blocks.  The bytes of those blocks are one contiguous
// range of the input and of the output, so the wave stages its input range into LDS with coalesced 16-byte loads, every
// lane runs the encoder's LFSR over its block's data part with the register file of the LFSR in LDS (codesize bytes
// as 32-bit words, lane stride an odd number of words: no bank conflicts on the state), and the output range leaves
// LDS the same way.  GF multiplication is a sum of logarithms looked up in an exp table: one LDS read per product.
//   encode: the output block is data || remainder;
//   check (repair): a stored block is a codeword iff the remainder of its data part equals its check bytes (iff every
//           syndrome is zero), so a clean block costs (n - codesize) * codesize products and only copies its data part;
//           any other block is listed for k_rs_fix and its data part is zero-filled for now (the failure result).
// k_rs_fix: one wave per listed block -- syndromes (lanes over roots, Horner), Berlekamp-Massey (lanes over locator
// coefficients, one wave reduction per step), Chien search over the block's own positions (lanes over positions),
// Forney (error values), then the syndromes of the corrected block are recomputed: only a block that is a codeword at
// distance <= codesize / 2 from what was stored is written back.  That makes the decoder an exact bounded-distance
// decoder, which is what reedsolo's rs_correct_msg computes.  Its state (syndromes, locator, evaluator) lives in LDS.
#include "../../include/frad_hip.h"
#include "frad_launch.hpp"

#include <map>
#include <mutex>
#include <vector>

namespace frad {

// per-codesize device table: exp[1024] (alpha^(i mod 255) for i < 510, zero above: the product with a zero factor
// is looked up at log + RS_ZERO), log[256], then the generator's coefficient logs lgg[256] as uint16 (RS_ZERO where
// g_j = 0 or j >= codesize)
constexpr int RS_EXP = 0, RS_LOG = 1024, RS_LGG = 1280, RS_TAB = 1792, RS_ZERO = 512;

__device__ __forceinline__ uint32_t gf_mul(const unsigned char* tab, uint32_t a, uint32_t b) {
    return (a && b) ? tab[RS_EXP + tab[RS_LOG + a] + tab[RS_LOG + b]] : 0u;
}

// frame of global block g: the last f with blk_off[f] <= g (blk_off non-decreasing, blk_off[0] = 0)
__device__ __forceinline__ long long rs_frame_of(const int64_t* __restrict__ blk_off, long long n_frames, long long g) {
    long long lo = 0, hi = n_frames;                      // invariant: blk_off[lo] <= g < blk_off[hi]
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (blk_off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

struct RsBlock { long long f, ip, op; int n, m; };

// geometry of global block g: input offset / length, output offset, data-part length m
template <int MODE>
__device__ __forceinline__ RsBlock rs_block(const int64_t* __restrict__ in_off, const int64_t* __restrict__ blk_off,
                                            const int64_t* __restrict__ out_off, long long n_frames, long long g, int dsize, int cs) {
    RsBlock b;
    b.f = rs_frame_of(blk_off, n_frames, g);
    const long long k = g - blk_off[b.f];
    const int bin = MODE == 0 ? dsize : dsize + cs, bout = MODE == 0 ? dsize + cs : dsize;
    const long long left = in_off[b.f + 1] - in_off[b.f] - k * bin;
    b.n = left < bin ? (int)left : bin;
    b.ip = in_off[b.f] + k * bin;
    b.op = out_off[b.f] + k * bout;
    b.m = MODE == 0 ? b.n : (b.n > cs ? b.n - cs : 0);
    return b;
}

template <int MODE>
__global__ void __launch_bounds__(64) k_rs_blocks(const unsigned char* __restrict__ in, const int64_t* __restrict__ in_off,
                                                  const int64_t* __restrict__ blk_off, const int64_t* __restrict__ out_off,
                                                  long long n_frames, long long n_blocks, int dsize, int cs,
                                                  const unsigned char* __restrict__ tables, unsigned char* __restrict__ out,
                                                  int32_t* __restrict__ work, int stage_in, int stage_out, int ws) {
    FRAD_DYN_SMEM(smem);
    unsigned char* tab = smem;
    const int lane = threadIdx.x;
    for (int i = lane; i < RS_TAB / 4; i += 64) reinterpret_cast<uint32_t*>(tab)[i] = reinterpret_cast<const uint32_t*>(tables)[i];
    unsigned char* sin = smem + RS_TAB;
    unsigned char* sout = sin + stage_in;
    uint32_t* state = reinterpret_cast<uint32_t*>(sout + stage_out) + lane * ws;
    const uint16_t* lgg = reinterpret_cast<const uint16_t*>(tab + RS_LGG);
    const long long in_total = in_off[n_frames], out_total = out_off[n_frames];
    const int W = (cs + 3) >> 2, top_w = (cs - 1) >> 2, top_s = ((cs - 1) & 3) * 8;
    team_sync<64>();
    for (long long g0 = (long long)blockIdx.x * 64; g0 < n_blocks; g0 += (long long)gridDim.x * 64) {
        const long long g = g0 + lane;
        const bool live = g < n_blocks;
        RsBlock b = rs_block<MODE>(in_off, blk_off, out_off, n_frames, live ? g : n_blocks - 1, dsize, cs);
        // the wave's input / output ranges: from its first block to the end of its last live block
        const u64 lo_in = wave_allreduce_u64(live ? (u64)b.ip : ~0ull, [](u64 x, u64 y) { return y < x ? y : x; });
        const u64 hi_in = wave_allreduce_u64(live ? (u64)(b.ip + b.n) : 0ull, [](u64 x, u64 y) { return y > x ? y : x; });
        const u64 lo_out = wave_allreduce_u64(live ? (u64)b.op : ~0ull, [](u64 x, u64 y) { return y < x ? y : x; });
        const u64 hi_out = wave_allreduce_u64(live ? (u64)(b.op + (MODE == 0 ? b.n + cs * (b.n > 0) : b.m)) : 0ull,
                                              [](u64 x, u64 y) { return y > x ? y : x; });
        const long long a_in = (long long)lo_in & ~15ll, a_out = (long long)lo_out & ~15ll;
        // coalesced stage-in: 16-byte pieces of the 16-aligned cover of [lo_in, hi_in), bytes at the buffer's end
        for (long long p = a_in + lane * 16; p < (long long)hi_in; p += 64 * 16) {
            unsigned char* dst = sin + (p - a_in);
            if (p + 16 <= in_total) {
                *reinterpret_cast<v4u*>(dst) = *reinterpret_cast<const v4u*>(in + p);
            } else {
                for (int i = 0; i < 16 && p + i < in_total; ++i) dst[i] = in[p + i];
            }
        }
        team_sync<64>();
        if (live) {
            const unsigned char* d = sin + (b.ip - a_in);
            unsigned char* o = sout + (b.op - a_out);
            for (int w = 0; w < W; ++w) state[w] = 0u;
            for (int k = 0; k < b.m; ++k) {
                const uint32_t c = d[k];
                if (MODE == 0) o[k] = (unsigned char)c;
                if (cs == 0) continue;
                const uint32_t fb = c ^ ((state[top_w] >> top_s) & 0xffu);
                // r_j <- r_(j-1) ^ fb * g_j: the register shifts up one byte, products of the feedback byte are added
                uint32_t carry = 0;
                if (fb == 0u) {
                    for (int w = 0; w < W; ++w) { const uint32_t x = state[w]; state[w] = (x << 8) | carry; carry = x >> 24; }
                } else {
                    const uint32_t lf = tab[RS_LOG + fb];
                    for (int w = 0; w < W; ++w) {
                        const uint32_t x = state[w];
                        const u64 l4 = *reinterpret_cast<const u64*>(lgg + 4 * w);
                        const uint32_t p = (uint32_t)tab[RS_EXP + lf + (uint32_t)(l4 & 0xffff)]
                                         | (uint32_t)tab[RS_EXP + lf + (uint32_t)((l4 >> 16) & 0xffff)] << 8
                                         | (uint32_t)tab[RS_EXP + lf + (uint32_t)((l4 >> 32) & 0xffff)] << 16
                                         | (uint32_t)tab[RS_EXP + lf + (uint32_t)(l4 >> 48)] << 24;
                        state[w] = ((x << 8) | carry) ^ p;
                        carry = x >> 24;
                    }
                }
            }
            if (MODE == 0) {
                if (b.n > 0)                                   // check bytes: r_(cs-1) first
                    for (int i = 0; i < cs; ++i) { const int j = cs - 1 - i; o[b.m + i] = (unsigned char)(state[j >> 2] >> ((j & 3) * 8)); }
            } else if (b.m > 0) {
                bool clean = true;
                for (int i = 0; i < cs; ++i) {
                    const int j = cs - 1 - i;
                    clean &= d[b.m + i] == (unsigned char)(state[j >> 2] >> ((j & 3) * 8));
                }
                if (clean) {
                    for (int k = 0; k < b.m; ++k) o[k] = d[k];
                } else {
                    for (int k = 0; k < b.m; ++k) o[k] = 0;
                    work[1 + atomicAdd(work, 1)] = (int32_t)g;
                }
            }
        }
        team_sync<64>();
        // coalesced stage-out; the pieces at both ends are shared with the neighbouring waves: bytes only
        for (long long p = a_out + lane * 16; p < (long long)hi_out; p += 64 * 16) {
            const unsigned char* src = sout + (p - a_out);
            if (p >= (long long)lo_out && p + 16 <= (long long)hi_out && p + 16 <= out_total) {
                *reinterpret_cast<v4u*>(out + p) = *reinterpret_cast<const v4u*>(src);
            } else {
                for (int i = 0; i < 16; ++i)
                    if (p + i >= (long long)lo_out && p + i < (long long)hi_out) out[p + i] = src[i];
            }
        }
        team_sync<64>();
    }
}

// syndromes S_i = r(alpha^i), i < cs, of the n bytes at blk (byte 0 = highest power); lanes over i.  Returns the OR of all.
__device__ __forceinline__ uint32_t rs_syndromes(const unsigned char* tab, const unsigned char* blk, int n, int cs, unsigned char* S) {
    uint32_t any = 0;
    for (int i = threadIdx.x; i < cs; i += 64) {
        uint32_t s = 0;
        for (int k = 0; k < n; ++k) s = (s ? tab[RS_EXP + tab[RS_LOG + s] + i] : 0u) ^ blk[k];
        if (S) S[i] = (unsigned char)s;
        any |= s;
    }
    return (uint32_t)wave_allreduce_u64(any, [](u64 x, u64 y) { return x | y; });
}

__global__ void __launch_bounds__(64) k_rs_fix(const unsigned char* __restrict__ in, const int64_t* __restrict__ in_off,
                                               const int64_t* __restrict__ blk_off, const int64_t* __restrict__ out_off,
                                               long long n_frames, int dsize, int cs, const unsigned char* __restrict__ tables,
                                               unsigned char* __restrict__ out, const int32_t* __restrict__ work,
                                               int32_t* __restrict__ corrected, int32_t* __restrict__ failed) {
    FRAD_DYN_SMEM(smem);
    unsigned char* tab = smem;
    const int lane = threadIdx.x;
    for (int i = lane; i < RS_LGG / 4; i += 64) reinterpret_cast<uint32_t*>(tab)[i] = reinterpret_cast<const uint32_t*>(tables)[i];
    unsigned char* blk = smem + RS_LGG;                    // [256] the block, corrected in place
    unsigned char* S = blk + 256;                          // [256] syndromes
    unsigned char* lam = S + 256;                          // [256] error locator Lambda (coefficient of x^j at j)
    unsigned char* B = lam + 256;                          // [256] BM's previous locator
    unsigned char* om = B + 256;                           // [256] error evaluator Omega = S Lambda mod x^cs
    team_sync<64>();
    const long long count = work[0];
    for (long long t = blockIdx.x; t < count; t += gridDim.x) {
        const long long g = work[1 + t];
        const RsBlock b = rs_block<1>(in_off, blk_off, out_off, n_frames, g, dsize, cs);
        const int n = b.n;
        for (int k = lane; k < 256; k += 64) { blk[k] = k < n ? in[b.ip + k] : 0; lam[k] = B[k] = om[k] = 0; }
        team_sync<64>();
        rs_syndromes(tab, blk, n, cs, S);
        if (lane == 0) { lam[0] = 1; B[0] = 1; }
        team_sync<64>();
        // Berlekamp-Massey: Lambda <- Lambda - (delta / bcoef) x^shift B
        int L = 0, shift = 1;
        uint32_t bcoef = 1;
        for (int r = 0; r < cs; ++r) {
            uint32_t part = 0;
            for (int j = lane; j <= L && j <= r; j += 64) part ^= gf_mul(tab, lam[j], S[r - j]);
            const uint32_t delta = (uint32_t)wave_allreduce_u64(part, [](u64 x, u64 y) { return x ^ y; });
            if (delta == 0) { ++shift; continue; }
            const uint32_t coef = tab[RS_EXP + tab[RS_LOG + delta] + 255 - tab[RS_LOG + bcoef]];
            unsigned char nl[4], old[4];
            for (int q = 0; q < 4; ++q) {
                const int j = lane + 64 * q;
                old[q] = lam[j];
                nl[q] = (unsigned char)(old[q] ^ (j >= shift ? gf_mul(tab, coef, B[j - shift]) : 0u));
            }
            team_sync<64>();
            const bool grow = 2 * L <= r;
            for (int q = 0; q < 4; ++q) {
                const int j = lane + 64 * q;
                if (grow) B[j] = old[q];
                lam[j] = nl[q];
            }
            if (grow) { L = r + 1 - L; bcoef = delta; shift = 1; } else { ++shift; }
            team_sync<64>();
        }
        bool ok = 2 * L <= cs;
        // Chien search over the block's own positions: byte k has location X = alpha^(n-1-k), a root of Lambda at 1/X
        uint32_t roots = 0;
        if (ok) {
            for (int k = lane; k < n; k += 64) {
                const int e = n - 1 - k, step = (255 - e) % 255;
                uint32_t v = 0;
                int acc = 0;                                   // j * step mod 255
                for (int j = 0; j <= L; ++j) {
                    const uint32_t c = lam[j];
                    if (c) { int idx = tab[RS_LOG + c] + acc; v ^= tab[RS_EXP + idx]; }
                    acc += step; if (acc >= 255) acc -= 255;
                }
                if (v == 0) ++roots;
                B[k] = v == 0;                                 // B is free after BM: error flags per position
            }
            for (int k = n + lane; k < 256; k += 64) B[k] = 0;
            roots = (uint32_t)wave_allreduce_u64(roots, [](u64 x, u64 y) { return x + y; });
            ok = (int)roots == L;
        }
        team_sync<64>();
        if (ok) {
            // Omega_i = sum_(j <= min(i, L)) Lambda_j S_(i-j), i < cs
            for (int i = lane; i < cs; i += 64) {
                uint32_t v = 0;
                for (int j = 0; j <= L && j <= i; ++j) v ^= gf_mul(tab, lam[j], S[i - j]);
                om[i] = (unsigned char)v;
            }
            team_sync<64>();
            // Forney, first consecutive root 0: Y = X Omega(1/X) / Lambda'(1/X)
            uint32_t bad = 0;
            for (int k = lane; k < n; k += 64) {
                if (!B[k]) continue;
                const int e = n - 1 - k, step = (255 - e) % 255;
                uint32_t o = 0, dl = 0;
                int acc = 0;                                   // log of (1/X)^i
                for (int i = 0; i < cs; ++i) {
                    if (om[i]) o ^= tab[RS_EXP + tab[RS_LOG + om[i]] + acc];
                    if ((i & 1) && i <= L && lam[i]) dl ^= tab[RS_EXP + tab[RS_LOG + lam[i]] + (acc >= step ? acc - step : acc + 255 - step)];
                    acc += step; if (acc >= 255) acc -= 255;
                }
                if (dl == 0) { bad = 1; continue; }
                const uint32_t y = o ? tab[RS_EXP + (tab[RS_LOG + o] + e + 255 - tab[RS_LOG + dl]) % 255] : 0u;
                blk[k] ^= (unsigned char)y;
            }
            ok = wave_allreduce_u64(bad, [](u64 x, u64 y) { return x | y; }) == 0;
            team_sync<64>();
            if (ok) ok = rs_syndromes(tab, blk, n, cs, nullptr) == 0;
        }
        if (ok)
            for (int k = lane; k < b.m; k += 64) out[b.op + k] = blk[k];
        if (lane == 0) atomicAdd(ok ? corrected + b.f : failed + b.f, 1);
        team_sync<64>();
    }
}

// ---- fixed-stride encode (frad_rs_encode_frames): n_frames payloads of the same length, frame f at in + f * in_stride, its
// protected form at out + f * out_stride.  Every frame has the same block count, so the work splits into units of 64
// consecutive blocks of one frame with no offset arrays.  One wave per unit, four waves per workgroup sharing one table:
//   stage-in:  the unit's input range (contiguous) with 4-byte loads into LDS, one row per block (row pitch an odd number of
//              dwords: the lanes' dword reads of their own rows hit 64 different banks);
//   LFSR:      one lane per block, the register file in VGPRs as WM dwords with the codesize bytes at the top (bytes below
//              4 WM - cs stay zero), one table row per data byte: prod[fb] = fb * g packed like the register, read as WM / 2
//              ds_read_b64, and the shift is a byte funnel across dwords -- WM / 2 LDS reads per data byte instead of cs
//              exp-table lookups;
//   stage-out: the check bytes go to a second LDS row per block and the unit's output range (contiguous) leaves as
//              data || check per block with 4-byte stores; bytes outside a frame's P output bytes are never written.
// When dsize, codesize and nbytes are multiples of 4 (`wide`, e.g. (96, 24) on 2048 x 2 x 32-bit payloads) no dword of the
// input or output range straddles two LDS rows, so both stages move dwords instead of bytes.
constexpr int RSF_WAVES = 4;

__device__ __forceinline__ uint32_t rsf_bswap(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

template <int WM>
__global__ void __launch_bounds__(256) k_rs_frames(const unsigned char* __restrict__ in, long long in_stride, long long n_frames,
                                                   long long nbytes, int dsize, int cs, const uint32_t* __restrict__ prod,
                                                   unsigned char* __restrict__ out, long long out_stride, long long nblk, long long upf,
                                                   int dpitch, int cpitch, int aligned_in, int aligned_out, int wide) {
    FRAD_DYN_SMEM(smem);
    uint32_t* tab = reinterpret_cast<uint32_t*>(smem);                      // [256][WM]
    for (int i = threadIdx.x; i < 256 * WM; i += blockDim.x) tab[i] = prod[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned char* sd = smem + 256 * WM * 4 + wave * 64 * (dpitch + cpitch);   // [64][dpitch] data rows
    unsigned char* sc = sd + 64 * dpitch;                                       // [64][cpitch] check rows
    const int bout = dsize + cs;
    const long long units = n_frames * upf;
    for (long long u = (long long)blockIdx.x * RSF_WAVES + wave; u < units; u += (long long)gridDim.x * RSF_WAVES) {
        const long long f = u / upf, k0 = (u - f * upf) * 64;
        const int nk = nblk - k0 < 64 ? (int)(nblk - k0) : 64;
        const long long left = nbytes - k0 * dsize;
        const int len_in = left < 64ll * dsize ? (int)left : 64 * dsize;
        const int m_last = len_in - (nk - 1) * dsize;                           // data bytes of the unit's last block
        const int len_out = len_in + nk * cs;
        const unsigned char* src = in + f * in_stride + k0 * dsize;             // k0 * dsize: a multiple of 64
        unsigned char* dst = out + f * out_stride + k0 * bout;
        for (int q = lane * 4; q < len_in; q += 256) {
            uint32_t w = 0;
            if (aligned_in && q + 4 <= len_in) w = *reinterpret_cast<const uint32_t*>(src + q);
            else for (int i = 0; i < 4 && q + i < len_in; ++i) w |= (uint32_t)src[q + i] << (8 * i);
            int b = q / dsize, r = q - b * dsize;
            if (wide) { *reinterpret_cast<uint32_t*>(sd + b * dpitch + r) = w; continue; }   // a dword never straddles two rows
            for (int i = 0; i < 4 && q + i < len_in; ++i) {
                sd[b * dpitch + r] = (unsigned char)(w >> (8 * i));
                if (++r == dsize) { r = 0; ++b; }
            }
        }
        team_sync<64>();
        if (lane < nk) {
            const int m = lane == nk - 1 ? m_last : dsize;
            const unsigned char* d = sd + lane * dpitch;
            uint32_t st[WM];
#pragma unroll
            for (int w = 0; w < WM; ++w) st[w] = 0u;
            auto step = [&](uint32_t c) {
                const uint32_t fb = (c ^ (st[WM - 1] >> 24)) & 0xffu;
                const v2u* row = reinterpret_cast<const v2u*>(tab + fb * WM);
#pragma unroll
                for (int h = WM / 2 - 1; h >= 0; --h) {
                    const v2u p = row[h];
                    const uint32_t below = h ? st[2 * h - 1] : 0u;
                    st[2 * h + 1] = ((st[2 * h + 1] << 8) | (st[2 * h] >> 24)) ^ p[1];
                    st[2 * h] = ((st[2 * h] << 8) | (below >> 24)) ^ p[0];
                }
            };
            int k = 0;
            for (; k + 4 <= m; k += 4) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(d + k);
                step(w); step(w >> 8); step(w >> 16); step(w >> 24);
            }
            for (; k < m; ++k) step(d[k]);
            uint32_t* c = reinterpret_cast<uint32_t*>(sc + lane * cpitch);    // check byte i = register byte 4 WM - 1 - i
#pragma unroll
            for (int w = 0; w < WM; ++w) c[WM - 1 - w] = rsf_bswap(st[w]);
        }
        team_sync<64>();
        for (int q = lane * 4; q < len_out; q += 256) {
            int b = q / bout, r = q - b * bout;
            uint32_t w = 0;
            const int n4 = len_out - q < 4 ? len_out - q : 4;
            if (wide) {                                                     // the dword lies in one data or one check row
                const int mb = b == nk - 1 ? m_last : dsize;
                w = r < mb ? *reinterpret_cast<const uint32_t*>(sd + b * dpitch + r) : *reinterpret_cast<const uint32_t*>(sc + b * cpitch + (r - mb));
            } else for (int i = 0; i < n4; ++i) {
                const int mb = b == nk - 1 ? m_last : dsize;
                const uint32_t v = r < mb ? sd[b * dpitch + r] : sc[b * cpitch + (r - mb)];
                w |= v << (8 * i);
                if (++r == mb + cs) { r = 0; ++b; }
            }
            if (aligned_out && n4 == 4) *reinterpret_cast<uint32_t*>(dst + q) = w;
            else for (int i = 0; i < n4; ++i) dst[q + i] = (unsigned char)(w >> (8 * i));
        }
        team_sync<64>();
    }
}

namespace {

std::mutex g_mu;
std::map<std::pair<int, int>, unsigned char*> g_tab;       // (device, codesize) -> table

int get_rs_tables(int cs, const unsigned char** out) {
    int dev = 0; FRAD_HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_tab.find({dev, cs});
    if (it != g_tab.end()) { *out = it->second; return FRAD_OK; }
    std::vector<unsigned char> h(RS_TAB, 0);
    unsigned x = 1;
    for (int i = 0; i < 255; ++i) {
        h[RS_EXP + i] = h[RS_EXP + i + 255] = (unsigned char)x;
        h[RS_LOG + x] = (unsigned char)i;
        x <<= 1;
        if (x & 0x100u) x ^= 0x11du;
    }
    auto mul = [&](unsigned a, unsigned b) -> unsigned { return (a && b) ? h[RS_EXP + h[RS_LOG + a] + h[RS_LOG + b]] : 0u; };
    std::vector<unsigned> gpoly(cs + 1, 0);                // coefficient of x^j at j
    gpoly[0] = 1;
    for (int i = 0; i < cs; ++i) {                         // times (x + alpha^i)
        const unsigned a = h[RS_EXP + i];
        for (int j = i + 1; j >= 1; --j) gpoly[j] = gpoly[j - 1] ^ mul(gpoly[j], a);
        gpoly[0] = mul(gpoly[0], a);
    }
    uint16_t* lgg = reinterpret_cast<uint16_t*>(h.data() + RS_LGG);
    for (int j = 0; j < 256; ++j) lgg[j] = (j < cs && gpoly[j]) ? h[RS_LOG + gpoly[j]] : (uint16_t)RS_ZERO;
    unsigned char* d = nullptr;
    FRAD_HIPCHK(hipMalloc(&d, RS_TAB));
    FRAD_HIPCHK(hipMemcpy(d, h.data(), RS_TAB, hipMemcpyHostToDevice));
    g_tab[{dev, cs}] = d; *out = d;
    return FRAD_OK;
}

int rs_grid(long long want) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
    const long long cap = 16ll * cus;
    return (int)(want < cap ? want : cap);
}

template <int MODE>
int rs_launch(const void* in, const int64_t* in_off, const int64_t* blk_off, const int64_t* out_off, int64_t n_frames, int64_t n_blocks,
              int32_t dsize, int32_t codesize, void* out, int32_t* work, void* stream) {
    const unsigned char* tables = nullptr;
    const int rc = get_rs_tables(codesize, &tables);
    if (rc != FRAD_OK) return rc;
    const int bin = MODE == 0 ? dsize : dsize + codesize, bout = MODE == 0 ? dsize + codesize : dsize;
    const int stage_in = (64 * bin + 32 + 15) / 16 * 16, stage_out = (64 * bout + 32 + 15) / 16 * 16;
    const int ws = ((codesize + 3) / 4) | 1;
    const size_t lds = (size_t)RS_TAB + stage_in + stage_out + 64u * 4u * ws;
    allow_lds(k_rs_blocks<MODE>, lds);
    hipLaunchKernelGGL(k_rs_blocks<MODE>, dim3((unsigned)rs_grid((n_blocks + 63) / 64)), dim3(64), lds, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned char*>(in), in_off, blk_off, out_off, (long long)n_frames, (long long)n_blocks,
                       (int)dsize, (int)codesize, tables, static_cast<unsigned char*>(out), work, stage_in, stage_out, ws);
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

int rs_check_args(const void* in, const int64_t* in_off, const int64_t* blk_off, const int64_t* out_off, int64_t n_frames,
                  int64_t n_blocks, void* out) {
    if (n_frames < 0 || n_blocks < 0 || n_blocks > 0x7ffffffell) return FRAD_E_INVALID;
    if (n_frames > 0 && (!in_off || !blk_off || !out_off)) return FRAD_E_INVALID;
    if (n_blocks > 0 && (!in || !out)) return FRAD_E_INVALID;
    if (!aligned16(in) || !aligned16(out)) return FRAD_E_INVALID;
    return FRAD_OK;
}


std::map<std::pair<int, int>, uint32_t*> g_prod;          // (device, codesize) -> fb * g rows of k_rs_frames

// register width of k_rs_frames for a codesize: an even number of dwords, from a short list of instantiations
int rsf_width(int cs) {
    static const int widths[] = {2, 4, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64};
    const int need = (cs + 3) / 4;
    for (int w : widths) if (w >= need) return w;
    return 64;
}

int get_rs_prod(int cs, const uint32_t** out) {
    int dev = 0; FRAD_HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_prod.find({dev, cs});
    if (it != g_prod.end()) { *out = it->second; return FRAD_OK; }
    unsigned char ex[512], lg[256] = {0};
    unsigned x = 1;
    for (int i = 0; i < 255; ++i) {
        ex[i] = ex[i + 255] = (unsigned char)x;
        lg[x] = (unsigned char)i;
        x <<= 1;
        if (x & 0x100u) x ^= 0x11du;
    }
    auto mul = [&](unsigned a, unsigned b) -> unsigned { return (a && b) ? ex[lg[a] + lg[b]] : 0u; };
    std::vector<unsigned> gpoly(cs + 1, 0);
    gpoly[0] = 1;
    for (int i = 0; i < cs; ++i) {
        const unsigned a = ex[i];
        for (int j = i + 1; j >= 1; --j) gpoly[j] = gpoly[j - 1] ^ mul(gpoly[j], a);
        gpoly[0] = mul(gpoly[0], a);
    }
    const int WM = rsf_width(cs), pad = 4 * WM - cs;
    std::vector<uint32_t> h((size_t)256 * WM, 0u);
    for (int fb = 0; fb < 256; ++fb)
        for (int j = 0; j < cs; ++j) {                     // register byte pad + j holds r_j
            const int a = pad + j;
            h[(size_t)fb * WM + a / 4] |= mul(fb, gpoly[j]) << (8 * (a & 3));
        }
    uint32_t* d = nullptr;
    FRAD_HIPCHK(hipMalloc(&d, h.size() * 4));
    FRAD_HIPCHK(hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    g_prod[{dev, cs}] = d; *out = d;
    return FRAD_OK;
}

template <int WM>
int rsf_launch(const unsigned char* in, long long in_stride, long long n_frames, long long nbytes, int dsize, int cs,
               unsigned char* out, long long out_stride, hipStream_t s) {
    const uint32_t* prod = nullptr;
    const int rc = get_rs_prod(cs, &prod);
    if (rc != FRAD_OK) return rc;
    const long long nblk = (nbytes + dsize - 1) / dsize, upf = (nblk + 63) / 64;
    const int dw = (dsize + 3) / 4, dpitch = 4 * (dw | 1), cpitch = 4 * (WM + 1);
    const size_t lds = (size_t)256 * WM * 4 + (size_t)RSF_WAVES * 64 * (dpitch + cpitch);
    const int aligned_in = ((reinterpret_cast<uintptr_t>(in) | (uintptr_t)in_stride) & 3u) == 0;
    const int aligned_out = ((reinterpret_cast<uintptr_t>(out) | (uintptr_t)out_stride) & 3u) == 0;
    const int wide = dsize % 4 == 0 && cs % 4 == 0 && nbytes % 4 == 0;     // rows and their boundaries are dword-aligned
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
    const long long want = (n_frames * upf + RSF_WAVES - 1) / RSF_WAVES, cap = 8ll * cus;
    allow_lds(k_rs_frames<WM>, lds);
    hipLaunchKernelGGL(k_rs_frames<WM>, dim3((unsigned)(want < cap ? want : cap)), dim3(64 * RSF_WAVES), lds, s, in, in_stride,
                       n_frames, nbytes, dsize, cs, prod, out, out_stride, nblk, upf, dpitch, cpitch, aligned_in, aligned_out, wide);
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

}  // namespace

void ecc_clear() {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_tab) (void)hipFree(kv.second);
    for (auto& kv : g_prod) (void)hipFree(kv.second);
    g_tab.clear();
    g_prod.clear();
}

}  // namespace frad

extern "C" int frad_rs_encode(const void* in, const int64_t* in_off, const int64_t* blk_off, const int64_t* out_off, int64_t n_frames,
                              int64_t n_blocks, int32_t dsize, int32_t codesize, void* out, void* stream) {
    using namespace frad;
    if (dsize < 1 || codesize < 0 || dsize + codesize > 255) return FRAD_E_INVALID;
    int rc = rs_check_args(in, in_off, blk_off, out_off, n_frames, n_blocks, out);
    if (rc != FRAD_OK || n_blocks == 0) return rc;
    return rs_launch<0>(in, in_off, blk_off, out_off, n_frames, n_blocks, dsize, codesize, out, nullptr, stream);
}

extern "C" int frad_rs_repair(const void* in, const int64_t* in_off, const int64_t* blk_off, const int64_t* out_off, int64_t n_frames,
                              int64_t n_blocks, int32_t dsize, int32_t codesize, void* out, int32_t* corrected, int32_t* failed,
                              int32_t* work, void* stream) {
    using namespace frad;
    if (dsize < 0 || codesize < 0 || dsize + codesize < 1 || dsize + codesize > 255) return FRAD_E_INVALID;
    int rc = rs_check_args(in, in_off, blk_off, out_off, n_frames, n_blocks, out);
    if (rc != FRAD_OK) return rc;
    if (n_frames > 0 && (!corrected || !failed)) return FRAD_E_INVALID;
    if (n_frames == 0) return FRAD_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FRAD_HIPCHK(hipMemsetAsync(corrected, 0, (size_t)n_frames * 4, s));
    FRAD_HIPCHK(hipMemsetAsync(failed, 0, (size_t)n_frames * 4, s));
    if (n_blocks == 0) return FRAD_OK;
    if (!work) return FRAD_E_INVALID;
    FRAD_HIPCHK(hipMemsetAsync(work, 0, 4, s));
    rc = rs_launch<1>(in, in_off, blk_off, out_off, n_frames, n_blocks, dsize, codesize, out, work, stream);
    if (rc != FRAD_OK) return rc;
    const unsigned char* tables = nullptr;
    rc = get_rs_tables(codesize, &tables);
    if (rc != FRAD_OK) return rc;
    const size_t lds = (size_t)RS_LGG + 5 * 256;
    hipLaunchKernelGGL(k_rs_fix, dim3((unsigned)rs_grid(n_blocks)), dim3(64), lds, s, static_cast<const unsigned char*>(in), in_off,
                       blk_off, out_off, (long long)n_frames, (int)dsize, (int)codesize, tables, static_cast<unsigned char*>(out),
                       static_cast<const int32_t*>(work), corrected, failed);
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}

extern "C" int frad_rs_encode_frames(const void* in, int64_t in_stride, int64_t n_frames, int64_t nbytes, int32_t dsize,
                                     int32_t codesize, void* out, int64_t out_stride, void* stream) {
    using namespace frad;
    if (dsize < 1 || codesize < 0 || dsize + codesize > 255 || n_frames < 0 || nbytes < 0) return FRAD_E_INVALID;
    const long long nblk = (nbytes + dsize - 1) / dsize, plen = nbytes + nblk * codesize;
    if (n_frames > 1 && (in_stride < nbytes || out_stride < plen)) return FRAD_E_INVALID;
    if (n_frames == 0 || nbytes == 0) return FRAD_OK;
    if (!in || !out) return FRAD_E_INVALID;
    const auto* i8 = static_cast<const unsigned char*>(in);
    auto* o8 = static_cast<unsigned char*>(out);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    switch (rsf_width(codesize)) {
        case 2: return rsf_launch<2>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 4: return rsf_launch<4>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 6: return rsf_launch<6>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 8: return rsf_launch<8>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 10: return rsf_launch<10>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 12: return rsf_launch<12>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 16: return rsf_launch<16>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 20: return rsf_launch<20>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 24: return rsf_launch<24>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 32: return rsf_launch<32>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        case 48: return rsf_launch<48>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
        default: return rsf_launch<64>(i8, in_stride, n_frames, nbytes, dsize, codesize, o8, out_stride, s);
    }
}
