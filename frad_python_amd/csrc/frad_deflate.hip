// frad_deflate.hip -- raw DEFLATE (RFC 1951) encode on the device: zlib.compressobj(-1, zlib.DEFLATED, -15) of the compact
// profiles' frame bodies (fourier/profile1.py:50, fourier/profile2.py:54), byte for byte.
//
//   k_deflate<GWIN>   one WAVE per frame.  The 64 lanes stage the body in LDS and clear the hash heads; one lane then runs
//                     zlib 1.2.x's level-6 compressor on it: deflate_slow (lazy matching; good 8, lazy 16, nice 128, chain
//                     128, TOO_FAR 4096, MAX_DIST 32 506) into a symbol buffer of lit_bufsize - 1 = 16 383 symbols
//                     (memLevel 8), then trees.c's _tr_flush_block per block: the heap with the `smaller` tie-break, the
//                     forced nodes of a code with fewer than two symbols, gen_bitlen's overflow fix, the code-length RLE of
//                     scan_tree / send_tree and the stored / fixed / dynamic choice.  What zlib computes is a sequential
//                     function of every earlier byte, so the parallelism is across frames.
//
// The hash chains: zlib links every position p <= len - 3 to the previous one of equal 15-bit hash.  A 32 768-entry head
// table per wave (64 KiB) would cost most of a CU's LDS, so the heads here are buckets of the hash's low DF_HB bits and the
// links join positions of equal bucket; a walk skips the positions whose full hash differs, which visits exactly zlib's
// chain (collisions of the full hash included) in zlib's order.  The links are prev[p & 32767], as zlib's, which is exact for
// bodies under wsize + MAX_DIST = 65 274 bytes: below that zlib never slides its window, and no link that a walk reads has
// been overwritten.  Longer bodies get status 1 (the caller deflates them on the host).
//
// LDS per wave: the tree workspace (DfTrees, ~4.5 KiB), the bucket heads (8 KiB), the links (2 B per position up to 32 768),
// the symbol buffer (3 B per symbol up to 16 384) and, when it fits in 160 KiB with the rest (GWIN = false), the body.  With
// GWIN = true (rows for bodies over about 30 KiB) the body is read from global memory instead.  The bit stream goes to the
// row as aligned 32-bit words (the tail bytewise); nothing is written past the stream's last byte.
#include "frad_common.hpp"
#include "frad_launch.hpp"
#include "../../include/frad_hip.h"

namespace frad {
namespace {

constexpr int DF_LIMIT = 65274;             // wsize + MAX_DIST: zlib slides its window from this length on
constexpr int DF_MAX_DIST = 32506;          // wsize - MIN_LOOKAHEAD
constexpr int DF_TOO_FAR = 4096;
constexpr int DF_LITBUF = 16384;            // lit_bufsize = 1 << (memLevel + 6); a block holds lit_bufsize - 1 symbols
constexpr int DF_HB = 12;                   // hash-bucket bits of the head table
constexpr int DF_HEAP = 573;                // HEAP_SIZE = 2 * L_CODES + 1
constexpr int L_CODES = 286, D_CODES = 30, BL_CODES = 19, END_BLOCK = 256;

struct Ct { uint16_t fc, dl; };             // zlib's ct_data: freq / code, dad / len
struct DfTrees {
    Ct ltree[DF_HEAP + 1];
    Ct dtree[2 * D_CODES + 1 + 3];
    Ct bltree[2 * BL_CODES + 1 + 1];
    uint16_t heap[DF_HEAP + 1];
    uint16_t bl_count[16];
    uint16_t next_code[16];
    unsigned char depth[DF_HEAP + 3];
};
constexpr int DF_TREES = ((int)sizeof(DfTrees) + 15) & ~15;

__host__ __device__ __forceinline__ long long df_bound(long long n) { return n + 6 * (n / (DF_LITBUF - 1) + 1) + 1; }

// the LDS layout for bodies of at most maxb bytes (offsets in bytes)
struct DfLayout { int head, prev, dbuf, lbuf, win, total; };
__host__ __device__ __forceinline__ DfLayout df_layout(int maxb, bool gwin) {
    DfLayout l;
    const int pn = maxb < 32768 ? maxb : 32768, sn = maxb < DF_LITBUF ? maxb : DF_LITBUF;
    l.head = DF_TREES;
    l.prev = l.head + 2 * (1 << DF_HB);
    l.dbuf = l.prev + ((2 * pn + 15) & ~15);
    l.lbuf = l.dbuf + ((2 * sn + 15) & ~15);
    l.win = l.lbuf + ((sn + 15) & ~15);
    l.total = l.win + (gwin ? 0 : ((maxb + 15) & ~15));
    return l;
}

// as team_sync<64>() but with workgroup-scope fences, which also wait for the wave's LDS traffic (s_waitcnt lgkmcnt(0)):
// the instruction sequence this kernel was verified with
__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ uint32_t df_rev(uint32_t v, int n) {             // the low n bits of v, reversed
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1u); v >>= 1; }
    return r;
}

// trees.c's static tables, computed
__device__ __forceinline__ int ext_lbits(int code) { return code < 8 || code == 28 ? 0 : (code - 4) >> 2; }
__device__ __forceinline__ int base_len(int code) { return code < 8 ? code : code == 28 ? 0 : (4 + (code & 3)) << ((code - 4) >> 2); }
__device__ __forceinline__ int length_code(int lc) {                          // _length_code[match length - 3]
    if (lc < 8) return lc;
    if (lc == 255) return 28;
    const int nb = 31 - __builtin_clz((unsigned)lc);
    return 4 * (nb - 2) + ((lc >> (nb - 2)) & 3) + 4;
}
__device__ __forceinline__ int ext_dbits(int code) { return code < 4 ? 0 : (code >> 1) - 1; }
__device__ __forceinline__ int base_dist(int code) { return code < 4 ? code : (2 + (code & 1)) << ((code >> 1) - 1); }
__device__ __forceinline__ int dist_code(int d) {                             // d_code(distance - 1)
    if (d < 4) return d;
    const int nb = 31 - __builtin_clz((unsigned)d);
    return 2 * nb + ((d >> (nb - 1)) & 1);
}
__device__ __forceinline__ int ext_blbits(int n) { return n == 16 ? 2 : n == 17 ? 3 : n == 18 ? 7 : 0; }
__device__ __forceinline__ int bl_order(int i) {                              // RFC 1951 3.2.7
    switch (i) {
        case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7;
        case 6: return 9; case 7: return 6; case 8: return 10; case 9: return 5; case 10: return 11; case 11: return 4;
        case 12: return 12; case 13: return 3; case 14: return 13; case 15: return 2; case 16: return 14; case 17: return 1;
        default: return 15;
    }
}
__device__ __forceinline__ int static_llen(int n) { return n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8; }
__device__ __forceinline__ uint32_t static_lcode(int n) {
    if (n < 144) return df_rev(0x30u + n, 8);
    if (n < 256) return df_rev(0x190u + (n - 144), 9);
    if (n < 280) return df_rev((uint32_t)(n - 256), 7);
    return df_rev(0xc0u + (n - 280), 8);
}

// one lane's compressor state; every array lives in LDS except `win` with GWIN and the output row
struct Deflater {
    const unsigned char* win;
    int len;
    uint16_t* head;
    uint16_t* prev;
    uint16_t* dbuf;
    unsigned char* lbuf;
    DfTrees* t;
    int last_lit, heap_len, heap_max;
    long long opt_len, static_len;
    u64 bb;                                    // bit buffer: bn pending bits, first bit in bit 0
    int bn;
    long long opos;
    unsigned char* row;

    __device__ __forceinline__ int hash(int p) const {
        return (((int)win[p] << 10) ^ ((int)win[p + 1] << 5) ^ (int)win[p + 2]) & 0x7fff;
    }
    // link p into its bucket (zlib's INSERT_STRING, buckets for heads); -> the bucket's previous head
    __device__ __forceinline__ int insert(int p, int h) {
        const int b = h & ((1 << DF_HB) - 1);
        const int q = head[b];
        prev[p & 32767] = (uint16_t)q;
        head[b] = (uint16_t)p;
        return q;
    }
    // from bucket entry q on, the first position of full hash h above `stop` (0: none)
    __device__ __forceinline__ int next_eq(int q, int h, int stop) const {
        while (q > stop && hash(q) != h) q = prev[q & 32767];
        return q > stop ? q : 0;
    }

    // ---- bit output
    __device__ __forceinline__ void put(uint32_t v, int n) {
        bb |= (u64)v << bn;
        bn += n;
        if (bn >= 32) {
            *FRAD_GPTR(uint32_t, row + opos) = (uint32_t)bb;
            opos += 4;
            bb >>= 32;
            bn -= 32;
        }
    }
    __device__ __forceinline__ void windup() { bn = (bn + 7) & ~7; if (bn >= 32) put(0, 0); }
    __device__ __forceinline__ void finish() {
        windup();
        for (int k = 0; k < bn; k += 8) row[opos++] = (unsigned char)(bb >> k);
        bn = 0;
    }

    // ---- trees.c
    __device__ __forceinline__ void init_block() {
        for (int n = 0; n < L_CODES; ++n) t->ltree[n].fc = 0;
        for (int n = 0; n < D_CODES; ++n) t->dtree[n].fc = 0;
        for (int n = 0; n < BL_CODES; ++n) t->bltree[n].fc = 0;
        t->ltree[END_BLOCK].fc = 1;
        opt_len = static_len = 0;
        last_lit = 0;
    }
    __device__ __forceinline__ bool smaller(const Ct* tree, int n, int m) const {
        return tree[n].fc < tree[m].fc || (tree[n].fc == tree[m].fc && t->depth[n] <= t->depth[m]);
    }
    __device__ __forceinline__ void pqdownheap(const Ct* tree, int k) {
        const int v = t->heap[k];
        int j = k << 1;
        while (j <= heap_len) {
            if (j < heap_len && smaller(tree, t->heap[j + 1], t->heap[j])) j++;
            if (smaller(tree, v, t->heap[j])) break;
            t->heap[k] = t->heap[j];
            k = j;
            j <<= 1;
        }
        t->heap[k] = (uint16_t)v;
    }
    // kind: 0 literal/length, 1 distance, 2 bit length
    __device__ __forceinline__ void gen_bitlen(Ct* tree, int max_code, int kind) {
        const int max_length = kind == 2 ? 7 : 15;
        for (int b = 0; b <= 15; ++b) t->bl_count[b] = 0;
        tree[t->heap[heap_max]].dl = 0;
        int overflow = 0, h;
        for (h = heap_max + 1; h < DF_HEAP; ++h) {
            const int n = t->heap[h];
            int bits = tree[tree[n].dl].dl + 1;
            if (bits > max_length) bits = max_length, overflow++;
            tree[n].dl = (uint16_t)bits;
            if (n > max_code) continue;
            t->bl_count[bits]++;
            int xbits = 0, slen = 0;
            if (kind == 0) { if (n >= 257) xbits = ext_lbits(n - 257); slen = static_llen(n); }
            else if (kind == 1) { xbits = ext_dbits(n); slen = 5; }
            else xbits = ext_blbits(n);
            const long long f = tree[n].fc;
            opt_len += f * (bits + xbits);
            if (kind != 2) static_len += f * (slen + xbits);
        }
        if (overflow == 0) return;
        do {
            int bits = max_length - 1;
            while (t->bl_count[bits] == 0) bits--;
            t->bl_count[bits]--;
            t->bl_count[bits + 1] += 2;
            t->bl_count[max_length]--;
            overflow -= 2;
        } while (overflow > 0);
        h = DF_HEAP;
        for (int bits = max_length; bits != 0; bits--) {
            int n = t->bl_count[bits];
            while (n != 0) {
                const int m = t->heap[--h];
                if (m > max_code) continue;
                if (tree[m].dl != bits) {
                    opt_len += ((long long)bits - tree[m].dl) * tree[m].fc;
                    tree[m].dl = (uint16_t)bits;
                }
                n--;
            }
        }
    }
    __device__ __forceinline__ void gen_codes(Ct* tree, int max_code) {
        uint16_t* next_code = t->next_code;
        uint32_t code = 0;
        for (int b = 1; b <= 15; ++b) { code = (code + t->bl_count[b - 1]) << 1; next_code[b] = (uint16_t)code; }
        for (int n = 0; n <= max_code; ++n) {
            const int l = tree[n].dl;
            if (l == 0) continue;
            tree[n].fc = (uint16_t)df_rev(next_code[l]++, l);
        }
    }
    __device__ __forceinline__ int build_tree(Ct* tree, int kind) {
        const int elems = kind == 0 ? L_CODES : kind == 1 ? D_CODES : BL_CODES;
        int max_code = -1;
        heap_len = 0;
        heap_max = DF_HEAP;
        for (int n = 0; n < elems; ++n) {
            if (tree[n].fc != 0) { t->heap[++heap_len] = (uint16_t)n; max_code = n; t->depth[n] = 0; }
            else tree[n].dl = 0;
        }
        while (heap_len < 2) {                                   // force at least two codes of non-zero frequency
            const int node = max_code < 2 ? ++max_code : 0;
            t->heap[++heap_len] = (uint16_t)node;
            tree[node].fc = 1;
            t->depth[node] = 0;
            opt_len--;
            if (kind == 0) static_len -= static_llen(node);
            else if (kind == 1) static_len -= 5;
        }
        for (int n = heap_len / 2; n >= 1; n--) pqdownheap(tree, n);
        int node = elems;
        do {
            const int n = t->heap[1];                            // pqremove
            t->heap[1] = t->heap[heap_len--];
            pqdownheap(tree, 1);
            const int m = t->heap[1];
            t->heap[--heap_max] = (uint16_t)n;
            t->heap[--heap_max] = (uint16_t)m;
            tree[node].fc = (uint16_t)(tree[n].fc + tree[m].fc);
            const int dn = t->depth[n], dm = t->depth[m];
            t->depth[node] = (unsigned char)((dn >= dm ? dn : dm) + 1);
            tree[n].dl = tree[m].dl = (uint16_t)node;
            t->heap[1] = (uint16_t)node++;
            pqdownheap(tree, 1);
        } while (heap_len >= 2);
        t->heap[--heap_max] = t->heap[1];
        gen_bitlen(tree, max_code, kind);
        gen_codes(tree, max_code);
        return max_code;
    }
    __device__ __forceinline__ void scan_tree(Ct* tree, int max_code) {
        int prevlen = -1, nextlen = tree[0].dl, count = 0, max_count = 7, min_count = 4;
        if (nextlen == 0) max_count = 138, min_count = 3;
        tree[max_code + 1].dl = 0xffff;                          // guard
        for (int n = 0; n <= max_code; ++n) {
            const int curlen = nextlen;
            nextlen = tree[n + 1].dl;
            if (++count < max_count && curlen == nextlen) continue;
            else if (count < min_count) t->bltree[curlen].fc += count;
            else if (curlen != 0) {
                if (curlen != prevlen) t->bltree[curlen].fc++;
                t->bltree[16].fc++;
            } else if (count <= 10) t->bltree[17].fc++;
            else t->bltree[18].fc++;
            count = 0;
            prevlen = curlen;
            if (nextlen == 0) max_count = 138, min_count = 3;
            else if (curlen == nextlen) max_count = 6, min_count = 3;
            else max_count = 7, min_count = 4;
        }
    }
    __device__ __forceinline__ void send_bl(int c) { put(t->bltree[c].fc, t->bltree[c].dl); }
    __device__ __forceinline__ void send_tree(const Ct* tree, int max_code) {
        int prevlen = -1, nextlen = tree[0].dl, count = 0, max_count = 7, min_count = 4;
        if (nextlen == 0) max_count = 138, min_count = 3;
        for (int n = 0; n <= max_code; ++n) {
            const int curlen = nextlen;
            nextlen = tree[n + 1].dl;
            if (++count < max_count && curlen == nextlen) continue;
            else if (count < min_count) { do { send_bl(curlen); } while (--count != 0); }
            else if (curlen != 0) {
                if (curlen != prevlen) { send_bl(curlen); count--; }
                send_bl(16); put((uint32_t)(count - 3), 2);
            } else if (count <= 10) { send_bl(17); put((uint32_t)(count - 3), 3); }
            else { send_bl(18); put((uint32_t)(count - 11), 7); }
            count = 0;
            prevlen = curlen;
            if (nextlen == 0) max_count = 138, min_count = 3;
            else if (curlen == nextlen) max_count = 6, min_count = 3;
            else max_count = 7, min_count = 4;
        }
    }
    template <bool STATIC>
    __device__ __forceinline__ void compress_block() {
        for (int lx = 0; lx < last_lit; ++lx) {
            int dist = dbuf[lx], lc = lbuf[lx];
            if (dist == 0) {
                if (STATIC) put(static_lcode(lc), static_llen(lc)); else put(t->ltree[lc].fc, t->ltree[lc].dl);
                continue;
            }
            int code = length_code(lc);
            if (STATIC) put(static_lcode(code + 257), static_llen(code + 257)); else put(t->ltree[code + 257].fc, t->ltree[code + 257].dl);
            int extra = ext_lbits(code);
            if (extra) put((uint32_t)(lc - base_len(code)), extra);
            dist--;
            code = dist_code(dist);
            if (STATIC) put(df_rev((uint32_t)code, 5), 5); else put(t->dtree[code].fc, t->dtree[code].dl);
            extra = ext_dbits(code);
            if (extra) put((uint32_t)(dist - base_dist(code)), extra);
        }
        if (STATIC) put(static_lcode(END_BLOCK), 7); else put(t->ltree[END_BLOCK].fc, t->ltree[END_BLOCK].dl);
    }
    // _tr_flush_block: bytes [bstart, bstart + stored_len) are the block's input
    __device__ __forceinline__ void flush_block(int bstart, int stored_len, bool last) {
        const int lmax = build_tree(t->ltree, 0);
        const int dmax = build_tree(t->dtree, 1);
        scan_tree(t->ltree, lmax);                               // build_bl_tree
        scan_tree(t->dtree, dmax);
        build_tree(t->bltree, 2);
        int max_blindex;
        for (max_blindex = BL_CODES - 1; max_blindex >= 3; max_blindex--)
            if (t->bltree[bl_order(max_blindex)].dl != 0) break;
        opt_len += 3 * ((long long)max_blindex + 1) + 5 + 5 + 4;
        long long opt_lenb = (opt_len + 3 + 7) >> 3;
        const long long static_lenb = (static_len + 3 + 7) >> 3;
        if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
        if (stored_len + 4 <= opt_lenb) {                        // _tr_stored_block
            put(last ? 1u : 0u, 3);
            windup();
            put((uint32_t)stored_len & 0xffffu, 16);
            put(~(uint32_t)stored_len & 0xffffu, 16);
            for (int i = 0; i < stored_len; ++i) put(win[bstart + i], 8);
        } else if (static_lenb == opt_lenb) {
            put((1u << 1) + (last ? 1u : 0u), 3);
            compress_block<true>();
        } else {
            put((2u << 1) + (last ? 1u : 0u), 3);
            put((uint32_t)(lmax + 1 - 257), 5);                  // send_all_trees
            put((uint32_t)(dmax + 1 - 1), 5);
            put((uint32_t)(max_blindex + 1 - 4), 4);
            for (int rank = 0; rank <= max_blindex; ++rank) put(t->bltree[bl_order(rank)].dl, 3);
            send_tree(t->ltree, lmax);
            send_tree(t->dtree, dmax);
            compress_block<false>();
        }
        init_block();
        if (last) finish();
    }
    // _tr_tally: -> the block is full
    __device__ __forceinline__ bool tally(int dist, int lc) {
        dbuf[last_lit] = (uint16_t)dist;
        lbuf[last_lit++] = (unsigned char)lc;
        if (dist == 0) t->ltree[lc].fc++;
        else {
            t->ltree[length_code(lc) + 257].fc++;
            t->dtree[dist_code(dist - 1)].fc++;
        }
        return last_lit == DF_LITBUF - 1;
    }

    // longest_match from chain head cur (prev_length < L); -> the best length (> prev_length when *start was set)
    __device__ __forceinline__ int longest_match(int cur, int h, int s, int L, int prev_length, int* start) const {
        int chain = prev_length >= 8 ? 128 >> 2 : 128;
        int best = prev_length;
        const int nice = L < 128 ? L : 128, maxm = L < 258 ? L : 258;
        const int limit = s > DF_MAX_DIST ? s - DF_MAX_DIST : 0;
        const unsigned char* scan = win + s;
        do {
            const unsigned char* m = win + cur;
            if (m[best] != scan[best] || m[best - 1] != scan[best - 1] || m[0] != scan[0] || m[1] != scan[1]) continue;
            int k = 2;
            while (k < maxm && m[k] == scan[k]) ++k;
            if (k > best) {
                *start = cur;
                best = k;
                if (k >= nice) break;
            }
        } while ((cur = next_eq(prev[cur & 32767], h, limit)) != 0 && --chain != 0);
        return best;
    }

    // deflate_slow over the whole body, then the final block
    __device__ __forceinline__ void run() {
        init_block();
        int strstart = 0, block_start = 0, match_length = 2, match_start = 0, match_available = 0;
        while (strstart < len) {
            const int L = len - strstart;
            int h = 0, hb = 0;
            if (L >= 3) { h = hash(strstart); hb = insert(strstart, h); }
            const int prev_length = match_length, prev_match = match_start;
            match_length = 2;
            if (L >= 3 && prev_length < 16 && prev_length < L) {
                const int head_at = next_eq(hb, h, strstart > DF_MAX_DIST ? strstart - DF_MAX_DIST - 1 : 0);
                if (head_at) {
                    match_length = longest_match(head_at, h, strstart, L, prev_length, &match_start);
                    if (match_length == 3 && strstart - match_start > DF_TOO_FAR) match_length = 2;
                }
            }
            if (prev_length >= 3 && match_length <= prev_length) {
                const bool bflush = tally(strstart - 1 - prev_match, prev_length - 3);
                const int max_insert = len - 3;
                for (int k = 1; k <= prev_length - 2; ++k) {
                    const int p = strstart + k;
                    if (p <= max_insert) insert(p, hash(p));
                }
                strstart += prev_length - 1;
                match_available = 0;
                match_length = 2;
                if (bflush) { flush_block(block_start, strstart - block_start, false); block_start = strstart; }
            } else if (match_available) {
                if (tally(0, win[strstart - 1])) { flush_block(block_start, strstart - block_start, false); block_start = strstart; }
                strstart++;
            } else {
                match_available = 1;
                strstart++;
            }
        }
        if (match_available) tally(0, win[strstart - 1]);
        flush_block(block_start, strstart - block_start, true);
    }
};

// One wave per frame: frame f is src[offs[f] .. offs[f+1]), deflated into dst + f * stride.  maxb: the longest body the
// launch's LDS holds.  Status 0: the row holds zlib's stream; 1: the body is 65 274 bytes or longer; 2: longer than maxb
// (the row is too small for its bound).  Nothing is written to the row with a non-zero status.
template <bool GWIN>
__global__ void __launch_bounds__(64) k_deflate(const unsigned char* __restrict__ src, const long long* __restrict__ offs,
                                                unsigned char* __restrict__ dst, long long stride, int maxb,
                                                long long* __restrict__ out_bytes, int32_t* __restrict__ status) {
    FRAD_DYN_SMEM(smem);
    const int lane = threadIdx.x;
    const long long f = blockIdx.x;
    const long long s0 = offs[f], n = offs[f + 1] - s0;
    const int st = n >= DF_LIMIT ? 1 : n > maxb ? 2 : 0;
    if (st) {
        if (lane == 0) { status[f] = st; out_bytes[f] = 0; }
        return;
    }
    const DfLayout lay = df_layout(maxb, GWIN);
    uint16_t* head = reinterpret_cast<uint16_t*>(smem + lay.head);
    for (int i = lane; i < (1 << DF_HB) / 2; i += 64) reinterpret_cast<uint32_t*>(head)[i] = 0u;
    unsigned char* win = smem + lay.win;
    if (!GWIN)
        for (long long i = lane; i < n; i += 64) win[i] = src[s0 + i];
    wsync();
    if (lane != 0) return;
    Deflater d;
    d.win = GWIN ? src + s0 : win;
    d.len = (int)n;
    d.head = head;
    d.prev = reinterpret_cast<uint16_t*>(smem + lay.prev);
    d.dbuf = reinterpret_cast<uint16_t*>(smem + lay.dbuf);
    d.lbuf = smem + lay.lbuf;
    d.t = reinterpret_cast<DfTrees*>(smem);
    d.bb = 0;
    d.bn = 0;
    d.opos = 0;
    d.row = dst + f * stride;
    d.run();
    status[f] = 0;
    out_bytes[f] = d.opos;
}

}  // namespace
}  // namespace frad

using namespace frad;

extern "C" int64_t frad_deflate_stride(int64_t max_body_bytes) {
    if (max_body_bytes < 0) return FRAD_E_INVALID;
    const long long n = max_body_bytes < DF_LIMIT ? max_body_bytes : DF_LIMIT - 1;
    return (df_bound(n) + 15) & ~15LL;
}

extern "C" int frad_deflate_raw(const void* src, const int64_t* src_offsets, int64_t n_frames, void* dst, int64_t dst_stride,
                                int64_t* dst_bytes, int32_t* status, void* stream) {
    if (n_frames < 0) return FRAD_E_INVALID;
    if (n_frames == 0) return FRAD_OK;
    if (!src || !src_offsets || !dst || !dst_bytes || !status) return FRAD_E_INVALID;
    if (dst_stride < 16 || (dst_stride & 15) || !aligned16(dst)) return FRAD_E_INVALID;
    if (n_frames > 0x7fffffffLL) return FRAD_E_UNSUPPORTED;
    // the longest body whose bound fits the row (and that zlib deflates without sliding its window)
    long long maxb = dst_stride - 7 - 6 * (dst_stride / (DF_LITBUF - 1) + 1);
    if (maxb > DF_LIMIT - 1) maxb = DF_LIMIT - 1;
    while (maxb > 0 && df_bound(maxb) > dst_stride) --maxb;
    while (maxb + 1 < DF_LIMIT && df_bound(maxb + 1) <= dst_stride) ++maxb;
    if (maxb < 0) maxb = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool gwin = df_layout((int)maxb, false).total > 160 * 1024;
    const size_t lds = (size_t)df_layout((int)maxb, gwin).total;
    if (gwin) {
        allow_lds(k_deflate<true>, lds);
        hipLaunchKernelGGL(k_deflate<true>, dim3((unsigned)n_frames), dim3(64), lds, s, static_cast<const unsigned char*>(src),
                           reinterpret_cast<const long long*>(src_offsets), static_cast<unsigned char*>(dst), (long long)dst_stride,
                           (int)maxb, reinterpret_cast<long long*>(dst_bytes), status);
    } else {
        allow_lds(k_deflate<false>, lds);
        hipLaunchKernelGGL(k_deflate<false>, dim3((unsigned)n_frames), dim3(64), lds, s, static_cast<const unsigned char*>(src),
                           reinterpret_cast<const long long*>(src_offsets), static_cast<unsigned char*>(dst), (long long)dst_stride,
                           (int)maxb, reinterpret_cast<long long*>(dst_bytes), status);
    }
    FRAD_HIPCHK(hipGetLastError());
    return FRAD_OK;
}
