// frad_inflate.hip -- raw DEFLATE (RFC 1951) decode on the device: the inflate of the compact profiles' frame bodies,
// zlib.decompress(frad, wbits=-15) in fourier/profile1.py:59 and fourier/profile2.py:61-64.
//
//   k_inflate<RING>   one WAVE per frame.  The bitstream is a sequential dependency, so the parallelism is across frames;
//                     inside a wave the 64 lanes share the work that splits: filling the Huffman lookup tables, match copies
//                     (lane j writes out[pos + j] from out[pos - dist + j % dist]: every source is older than the copy, so an
//                     overlapping copy needs no serial loop), stored blocks (64 bytes per step), staging the input and the
//                     coalesced write-out of the window.  The symbol decode itself is wave-uniform: every lane runs the same
//                     bit reader on the same LDS words.
//
// LDS per wave: the input (a ring of 2 KiB of 32-bit words, refilled from global memory by the lanes), the code lengths,
// the primary tables (10 bits for literal/length codes, 8 for distance codes, 7 for the code-length code) with the symbols
// sorted by code length behind them, and the output window.  A code longer than the primary table's bits is resolved from
// those sorted symbols: the codes of one length are consecutive integers (canonical Huffman), so the sorted list is the
// concatenation of one sub-table per length, indexed by code - first code of that length.
// The window is the whole output row when the row is at most 32 KiB (RING = false: the row never wraps, back references
// index it directly) and otherwise a 32 KiB ring (RING = true), written to the row in 16 KiB pieces as it fills.  Back
// references never read global memory.
//
// Acceptance is zlib's (inflate.c / inftrees.c): BTYPE 3, a stored LEN / NLEN mismatch, HLIT > 286 or HDIST > 30, a repeat
// code 16 with no previous length, repeats past HLIT + HDIST, an over-subscribed code, an incomplete code (permitted only for
// a literal/length or distance code whose single code has length 1, never for the code-length code; an empty code is
// accepted and fails when a symbol is decoded from it), no end-of-block code, literal/length symbols 286-287, distance
// symbols 30-31, a distance beyond the bytes produced, and input that ends before the final block's end-of-block are all
// status 1.  Bytes after the final block are ignored.  Status 2: the output would not fit the row.
#include "frad_common.hpp"
#include "frad_host.hpp"
#include "../../include/frad_hip.h"

namespace frad {
namespace {

constexpr int IF_LROOT = 10;               // primary table bits: literal/length
constexpr int IF_DROOT = 8;                //                     distance
constexpr int IF_CROOT = 7;                //                     code-length code (its codes are at most 7 bits)
constexpr int IF_IW = 512;                 // input ring, 32-bit words (2 KiB)
constexpr int IF_RING = 32768;             // the DEFLATE window; RING = true keeps the last 32 KiB of the output
constexpr int IF_FLUSH = 16384;            // RING = true: bytes per write-out of the ring
constexpr int IF_DIST_AT = 288;            // code lengths: literal/length at [0, 288), distance at [288, 320)

// LDS layout (bytes, every offset a multiple of 16)
struct HTab { int32_t first[16], cnt[16], offs[16], maxlen, pad[3]; };   // per code length: first code, count, offset in the sorted list
constexpr int L_LENS = 0;                                  // u8 [320]
constexpr int L_CLENS = L_LENS + 320;                      // u8 [32]: the code-length code's 19 lengths
constexpr int L_LTAB = L_CLENS + 32;                       // u16 [1 << IF_LROOT] (the code-length table uses its first 128)
constexpr int L_DTAB = L_LTAB + 2 * (1 << IF_LROOT);       // u16 [1 << IF_DROOT]
constexpr int L_LWORK = L_DTAB + 2 * (1 << IF_DROOT);      // u16 [288] symbols sorted by (length, symbol)
constexpr int L_DWORK = L_LWORK + 2 * 288;                 // u16 [32]
constexpr int L_LH = L_DWORK + 2 * 32;                     // HTab (literal/length, and the code-length code before it)
constexpr int L_DH = L_LH + (int)sizeof(HTab);             // HTab (distance)
constexpr int L_IN = L_DH + (int)sizeof(HTab);             // u32 [IF_IW]
constexpr int L_WIN = L_IN + 4 * IF_IW;                    // output window
static_assert(L_WIN % 16 == 0 && sizeof(HTab) % 16 == 0, "LDS layout");

__device__ __forceinline__ uint32_t bitrev(uint32_t v, int n) {            // the low n bits of v, reversed
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - n);
}

__device__ __forceinline__ int clen_order(int i) {                         // RFC 1951 3.2.7
    switch (i) {
        case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7;
        case 6: return 9; case 7: return 6; case 8: return 10; case 9: return 5; case 10: return 11; case 11: return 4;
        case 12: return 12; case 13: return 3; case 14: return 13; case 15: return 2; case 16: return 14; case 17: return 1;
        default: return 15;
    }
}

// Build the decode structures of the code whose lengths are lens[0 .. 4*nwords) (zero past the alphabet).  All 64 lanes
// call it.  Returns false where zlib's inflate_table refuses the lengths (over-subscribed; incomplete unless `lenient` and
// the only code has length 1).  An empty code builds (every lookup then fails), as in zlib.
// Primary entry e (the next ROOT input bits, first bit in bit 0): (symbol << 4) | length, or 0 = no code of <= ROOT bits.
template <int ROOT>
__device__ __forceinline__ bool build_code(const unsigned char* lens, int nwords, bool lenient, HTab* h, unsigned short* tab,
                                           unsigned short* work, int lane) {
    team_sync<64>();                                                   // the previous block's lookups are done
    const uint32_t* l32 = reinterpret_cast<const uint32_t*>(lens);
    // lane l (1..15) counts the codes of length l: four lengths per (broadcast) LDS read
    int cnt = 0;
    for (int w = 0; w < nwords; ++w) {
        const uint32_t v = l32[w];
        cnt += ((int)(v & 255u) == lane) + ((int)((v >> 8) & 255u) == lane) + ((int)((v >> 16) & 255u) == lane) + ((int)(v >> 24) == lane);
    }
    if (lane >= 1 && lane < 16) h->cnt[lane] = cnt;
    team_sync<64>();
    int left = 1, maxl = 0, code = 0, off = 0, my_first = 0, my_off = 0;
    bool over = false;
    for (int l = 1; l < 16; ++l) {                             // uniform: the same 15 broadcast reads in every lane
        const int c = h->cnt[l];
        left = 2 * left - c;
        over |= left < 0;
        if (c) maxl = l;
        if (l == lane) { my_first = code; my_off = off; }
        code = (code + c) << 1;
        off += c;
    }
    if (over || (left > 0 && maxl > 0 && !(lenient && maxl == 1))) return false;
    if (lane >= 1 && lane < 16) { h->first[lane] = my_first; h->offs[lane] = my_off; }
    if (lane == 0) h->maxlen = maxl;
    // sorted symbols: lane l places the symbols of length l, in symbol order
    {
        int at = my_off;
        for (int w = 0; w < nwords; ++w) {
            const uint32_t v = l32[w];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if ((int)((v >> (8 * b)) & 255u) == lane && lane != 0) work[at++] = (unsigned short)(4 * w + b);
        }
    }
    team_sync<64>();
    // primary table: entry e holds the code of <= ROOT bits that is a prefix of e's bits, found per length (lanes split
    // the entries, the lengths are uniform)
    constexpr int PER = (1 << ROOT) / 64;
    uint32_t ent[PER], r[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) { ent[k] = 0; r[k] = bitrev((uint32_t)(lane + 64 * k), ROOT); }
    const int top = maxl < ROOT ? maxl : ROOT;
    for (int l = 1; l <= top; ++l) {
        const int c = h->cnt[l], f = h->first[l], o = h->offs[l];
        if (!c) continue;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int idx = (int)(r[k] >> (ROOT - l)) - f;
            if (ent[k] == 0 && idx >= 0 && idx < c) ent[k] = ((uint32_t)work[o + idx] << 4) | (uint32_t)l;
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) tab[lane + 64 * k] = (unsigned short)ent[k];
    team_sync<64>();
    return true;
}

// decode one symbol from the next input bits `b` (first bit in bit 0, >= 15 valid); -> symbol, *len its code length,
// or -1 (no such code: an unused code of an incomplete or empty code)
template <int ROOT>
__device__ __forceinline__ int decode_sym(uint32_t b, const HTab* h, const unsigned short* tab, const unsigned short* work, int* len) {
    const uint32_t e = tab[b & ((1u << ROOT) - 1)];
    if (e) { *len = (int)(e & 15u); return (int)(e >> 4); }
    const int maxl = h->maxlen;
    const uint32_t r = bitrev(b & 0x7fffu, 15);
    for (int l = ROOT + 1; l <= maxl; ++l) {                   // the codes longer than the primary table
        const int idx = (int)(r >> (15 - l)) - h->first[l];
        if (idx >= 0 && idx < h->cnt[l]) { *len = l; return work[h->offs[l] + idx]; }
    }
    return -1;
}

// One wave per frame: frame f is src[offs[f] .. offs[f+1]), inflated into dst + f * stride (capacity = stride bytes).
// wbytes: the LDS window (RING = false: stride; RING = true: IF_RING).
template <bool RING>
__global__ void __launch_bounds__(64) k_inflate(const unsigned char* __restrict__ src, const long long* __restrict__ offs,
                                                unsigned char* __restrict__ dst, long long stride, long long* __restrict__ out_bytes,
                                                int32_t* __restrict__ status) {
    FRAD_DYN_SMEM(smem);
    const int lane = threadIdx.x;
    const long long f = blockIdx.x;
    const long long s0 = offs[f], len = offs[f + 1] - s0;
    const unsigned char* in = src + s0;
    unsigned char* row = dst + f * stride;
    const long long cap = stride;
    unsigned char* lens = smem + L_LENS;
    unsigned char* clens = smem + L_CLENS;
    unsigned short* ltab = reinterpret_cast<unsigned short*>(smem + L_LTAB);
    unsigned short* dtab = reinterpret_cast<unsigned short*>(smem + L_DTAB);
    unsigned short* lwork = reinterpret_cast<unsigned short*>(smem + L_LWORK);
    unsigned short* dwork = reinterpret_cast<unsigned short*>(smem + L_DWORK);
    HTab* lh = reinterpret_cast<HTab*>(smem + L_LH);
    HTab* dh = reinterpret_cast<HTab*>(smem + L_DH);
    uint32_t* in32 = reinterpret_cast<uint32_t*>(smem + L_IN);
    const unsigned char* in8 = smem + L_IN;
    unsigned char* win = smem + L_WIN;
    constexpr long long WMASK = RING ? IF_RING - 1 : ~0LL;

    // ---- input: word k = bytes [4k, 4k + 4) of the frame, zero past its end; 4 zero words of tail so that a peek never
    // leaves the loaded range.  Read bytewise: nothing outside [offs[f], offs[f+1]) is touched.
    const long long nin = (len + 3) / 4 + 4;
    long long whi = 0;                                         // words [whi - IF_IW, whi) are in the ring (uniform)
    auto need = [&](long long lo, long long hi) {              // words [lo, hi) must be loaded; hi - lo <= IF_IW
        if (whi >= hi || whi >= nin) return;
        const long long nh = lo + IF_IW < nin ? lo + IF_IW : nin;
        team_sync<64>();                                               // every lane is done with the words being replaced
        for (long long k = (whi > lo ? whi : lo) + lane; k < nh; k += 64) {
            const long long b = 4 * k;
            uint32_t v = 0;
            if (b + 3 < len) v = (uint32_t)in[b] | ((uint32_t)in[b + 1] << 8) | ((uint32_t)in[b + 2] << 16) | ((uint32_t)in[b + 3] << 24);
            else
                for (int j = 0; j < 4; ++j) v |= (b + j < len ? (uint32_t)in[b + j] : 0u) << (8 * j);
            in32[k & (IF_IW - 1)] = v;
        }
        whi = nh;
        team_sync<64>();
    };
    auto peek = [&](long long bp) -> uint32_t {                // 32 input bits from bit bp (loaded: words bp/32 and bp/32 + 1)
        const long long w = bp >> 5;
        const u64 v = ((u64)in32[(w + 1) & (IF_IW - 1)] << 32) | (u64)in32[w & (IF_IW - 1)];
        return (uint32_t)(v >> (bp & 31));
    };

    long long pos = 0, flushed = 0, fenced = 0, bp = 0;
    const long long nbits = 8 * len;
    int st = len > 0 ? 0 : 1;
    int tabs = 0;                                              // 1: the fixed code's tables are built
    // RING: write ring bytes [flushed, flushed + n) to the row (flushed and the row 16-byte aligned)
    auto write_out = [&](long long n) {
        team_sync<64>();
        const long long full = n & ~15LL;
        for (long long j = 16 * lane; j < full; j += 1024) {
            const v4u v = *reinterpret_cast<const v4u*>(win + ((flushed + j) & WMASK));
            *FRAD_GPTR(v4u, row + flushed + j) = v;
        }
        if (lane < n - full) row[flushed + full + lane] = win[(flushed + full + lane) & WMASK];
        flushed += n;
        fenced = pos;                                          // (the barrier above made every byte so far visible)
        team_sync<64>();                                               // the ring bytes written out may now be overwritten
    };
    bool last = false;
    while (st == 0 && !last) {
        need(bp >> 5, (bp >> 5) + 4);
        const uint32_t hdr = peek(bp);
        last = hdr & 1u;
        const int type = (int)((hdr >> 1) & 3u);
        bp += 3;
        if (type == 3) { st = 1; break; }
        if (type == 0) {                                       // ---- stored block
            bp = (bp + 7) & ~7LL;
            need(bp >> 5, (bp >> 5) + 4);
            const uint32_t ln = peek(bp);
            const long long n = ln & 0xffffu;
            if ((ln >> 16) != (uint32_t)(~n & 0xffff)) { st = 1; break; }
            bp += 32;
            const long long p = bp >> 3;
            if (p + n > len) { st = 1; break; }
            if (pos + n > cap) { st = 2; break; }
            for (long long o = 0; o < n; o += 64) {
                if (RING && pos - flushed >= IF_FLUSH) write_out(IF_FLUSH);
                need((p + o) >> 2, ((p + o) >> 2) + 18);
                if (o + lane < n) win[(pos + lane) & WMASK] = in8[(p + o + lane) & (4 * IF_IW - 1)];
                pos += n - o < 64 ? n - o : 64;
            }
            bp += 8 * n;
            continue;
        }
        HTab* const dhp = dh;
        if (type == 1) {                                       // ---- fixed code
            if (tabs != 1) {
                team_sync<64>();
                for (int i = lane; i < 320; i += 64) lens[i] = (unsigned char)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
                build_code<IF_LROOT>(lens, 72, true, lh, ltab, lwork, lane);
                build_code<IF_DROOT>(lens + IF_DIST_AT, 8, true, dhp, dtab, dwork, lane);
                tabs = 1;
            }
        } else {                                               // ---- dynamic code
            tabs = 0;
            need(bp >> 5, (bp >> 5) + 4);
            const uint32_t h14 = peek(bp);
            const int nlen = (int)(h14 & 31u) + 257, ndist = (int)((h14 >> 5) & 31u) + 1, ncode = (int)((h14 >> 10) & 15u) + 4;
            bp += 14;
            if (nlen > 286 || ndist > 30) { st = 1; break; }
            team_sync<64>();                                           // (the previous block's tables and lengths are no longer read)
            for (int i = lane; i < 320; i += 64) lens[i] = 0;
            if (lane < 32) clens[lane] = 0;
            team_sync<64>();
            for (int i = 0; i < ncode; ++i) {                  // uniform; lane 0 stores
                need(bp >> 5, (bp >> 5) + 4);
                const uint32_t c3 = peek(bp) & 7u;
                if (lane == 0) clens[clen_order(i)] = (unsigned char)c3;
                bp += 3;
            }
            team_sync<64>();
            if (!build_code<IF_CROOT>(clens, 5, false, lh, ltab, lwork, lane)) { st = 1; break; }
            int have = 0, prev = -1;
            const int total = nlen + ndist;
            while (have < total) {
                if (bp > nbits) { st = 1; break; }
                need(bp >> 5, (bp >> 5) + 4);
                uint32_t b = peek(bp);
                int cl = 0;
                const int sym = decode_sym<IF_CROOT>(b, lh, ltab, lwork, &cl);
                if (sym < 0) { st = 1; break; }
                bp += cl;
                b >>= cl;
                int val, rep;
                if (sym < 16) { val = sym; rep = 1; }
                else if (sym == 16) {
                    if (prev < 0) { st = 1; break; }
                    val = prev; rep = 3 + (int)(b & 3u); bp += 2;
                } else if (sym == 17) { val = 0; rep = 3 + (int)(b & 7u); bp += 3; }
                else { val = 0; rep = 11 + (int)(b & 127u); bp += 7; }
                if (have + rep > total) { st = 1; break; }
                for (int j = lane; j < rep; j += 64) {
                    const int i = have + j;
                    lens[i < nlen ? i : IF_DIST_AT + (i - nlen)] = (unsigned char)val;
                }
                have += rep;
                prev = val;
            }
            if (st) break;
            team_sync<64>();
            if (lens[256] == 0) { st = 1; break; }             // no end-of-block code
            if (!build_code<IF_LROOT>(lens, 72, true, lh, ltab, lwork, lane)) { st = 1; break; }
            if (!build_code<IF_DROOT>(lens + IF_DIST_AT, 8, true, dhp, dtab, dwork, lane)) { st = 1; break; }
        }
        // ---- Huffman-coded data
        for (;;) {
            if (bp > nbits) { st = 1; break; }                 // the input ended inside the last symbol
            if (RING && pos - flushed >= IF_FLUSH) write_out(IF_FLUSH);
            need(bp >> 5, (bp >> 5) + 4);
            uint32_t b = peek(bp);
            int cl = 0;
            const int sym = decode_sym<IF_LROOT>(b, lh, ltab, lwork, &cl);
            if (sym < 0 || sym > 285) { st = 1; break; }
            bp += cl;
            if (sym < 256) {
                if (pos >= cap) { st = 2; break; }
                if (lane == (int)(pos & 63)) win[pos & WMASK] = (unsigned char)sym;
                ++pos;
                continue;
            }
            if (sym == 256) break;
            b >>= cl;
            int mlen;
            if (sym < 265) mlen = sym - 254;
            else if (sym == 285) mlen = 258;
            else {
                const int e = (sym - 261) >> 2;
                mlen = ((((sym - 265) & 3) + 4) << e) + 3 + (int)(b & ((1u << e) - 1u));
                bp += e;
            }
            const uint32_t db = peek(bp);                      // (<= 20 bits consumed since the 4-word load: still loaded)
            int dl = 0;
            const int dsym = decode_sym<IF_DROOT>(db, dhp, dtab, dwork, &dl);
            if (dsym < 0 || dsym > 29) { st = 1; break; }
            bp += dl;
            long long dist;
            if (dsym < 4) dist = dsym + 1;
            else {
                const int e = (dsym >> 1) - 1;
                dist = (long long)(((2 + (dsym & 1)) << e) + 1) + (long long)((db >> dl) & ((1u << e) - 1u));
                bp += e;
            }
            if (dist > pos) { st = 1; break; }
            if (pos + mlen > cap) { st = 2; break; }
            // every source byte is older than this copy; make the ones written since the last fence visible to all lanes
            if (pos - dist + (dist < mlen ? dist : mlen) > fenced) { team_sync<64>(); fenced = pos; }
            unsigned char v[5];
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int j = lane + 64 * t;
                v[t] = j < mlen ? win[(pos - dist + (dist >= mlen ? j : j % (int)dist)) & WMASK] : 0;
            }
            if (RING) team_sync<64>();                                 // a ring slot read above may be one this copy writes
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int j = lane + 64 * t;
                if (j < mlen) win[(pos + j) & WMASK] = v[t];
            }
            pos += mlen;
        }
    }
    if (st == 0 && bp > nbits) st = 1;                         // the final end-of-block lies past the input
    if (st == 0) {
        if (RING) write_out(pos - flushed);
        else {
            team_sync<64>();
            const long long full = pos & ~15LL;
            for (long long j = 16 * lane; j < full; j += 1024) *FRAD_GPTR(v4u, row + j) = *reinterpret_cast<const v4u*>(win + j);
            if (lane < pos - full) row[full + lane] = win[full + lane];
        }
    }
    if (lane == 0) { status[f] = st; out_bytes[f] = st == 0 ? pos : 0; }
}

}  // namespace
}  // namespace frad

using namespace frad;

extern "C" int frad_inflate_raw(const void* src, const int64_t* src_offsets, int64_t n_frames, void* dst, int64_t dst_stride,
                                int64_t* dst_bytes, int32_t* status, void* stream) {
    if (n_frames < 0) return FRAD_E_INVALID;
    if (n_frames == 0) return FRAD_OK;
    if (!src || !src_offsets || !dst || !dst_bytes || !status) return FRAD_E_INVALID;
    if (dst_stride < 16 || (dst_stride & 15) || !aligned16(dst)) return FRAD_E_INVALID;
    if (n_frames > 0x7fffffffLL) return FRAD_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool ring = dst_stride > IF_RING;
    const size_t lds = (size_t)L_WIN + (size_t)(ring ? IF_RING : dst_stride);
    if (ring)
        hipLaunchKernelGGL(k_inflate<true>, dim3((unsigned)n_frames), dim3(64), lds, s, static_cast<const unsigned char*>(src),
                           reinterpret_cast<const long long*>(src_offsets), static_cast<unsigned char*>(dst), (long long)dst_stride,
                           reinterpret_cast<long long*>(dst_bytes), status);
    else
        hipLaunchKernelGGL(k_inflate<false>, dim3((unsigned)n_frames), dim3(64), lds, s, static_cast<const unsigned char*>(src),
                           reinterpret_cast<const long long*>(src_offsets), static_cast<unsigned char*>(dst), (long long)dst_stride,
                           reinterpret_cast<long long*>(dst_bytes), status);
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}
