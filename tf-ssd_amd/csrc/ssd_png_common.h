// What the device PNG encoder's kernels and its host model (both in ssd_png.hip) share: the stream format of
// include/ssd_hip.h ("PNG ENCODER") as step functions.  A segment of the filtered stream is coded by 256 "threads" that
// each own a 64-byte piece and run the same phases in the same order; a phase reads only what earlier phases wrote, so the
// kernel runs phase(t) on thread t with a barrier behind it and the host model runs it as a loop over t.  Whatever threads
// share is summed or ORed (integer, commutative), so the bytes do not depend on the order the threads run in.
// Integer arithmetic only.
#pragma once
#include "common.h"

namespace ssd {

enum : int {
    kPngSeg = 16384,                    // bytes of filtered stream per segment = per deflate block = per IDAT chunk
    kPngThreads = 256,                  // "threads" of a segment
    kPngPiece = kPngSeg / kPngThreads,  // bytes of the segment a thread walks
    kPngSlot = kPngSeg + 16,            // a segment's finished chunk data at the worst: 78 9C + a stored header + the bytes
    kPngCrcPiece = 68,                  // bytes of the finished data a thread takes the CRC of: 256 x 68 >= kPngSlot
    kPngFrontBytes = 33,                // the signature and IHDR
    kPngLit = 286,                      // literal / length symbols; HLIT is always 29
    kPngSeq = 287,                      // code lengths the block header carries: those and the one distance code
    kPngCl = 19,                        // code-length symbols; HCLEN is always 15
    kPngNone = 2 * kPngSeg,             // "no run starts in this piece"
};
static const unsigned kPngCrcPoly = 0xEDB88320u;
static const unsigned kPngAdlerMod = 65521u;

#define SSD_PNG_HD __host__ __device__ __forceinline__

// ---- rule 1: the filtered stream -------------------------------------------------------------------------------------
SSD_PNG_HD int png_abs(const int v) { return v < 0 ? -v : v; }
SSD_PNG_HD int png_paeth(const int a, const int b, const int c) {
    const int p = a + b - c, pa = png_abs(p - a), pb = png_abs(p - b), pc = png_abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// x filtered with `type` 0..4; a: the byte 3 to the left, b: the byte above, c: the byte above a (0 outside the image)
SSD_PNG_HD unsigned png_filter(const int type, const int x, const int a, const int b, const int c) {
    const int pred = type == 0 ? 0 : (type == 1 ? a : (type == 2 ? b : (type == 3 ? (a + b) >> 1 : png_paeth(a, b, c))));
    return (unsigned)(x - pred) & 255u;
}
SSD_PNG_HD unsigned png_cost(const unsigned v) { return v < 128u ? v : 256u - v; }
// the adaptive choice: the least sum, ties to the lowest type
SSD_PNG_HD int png_pick_filter(const unsigned* sums) {
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (sums[t] < sums[best]) best = t;
    return best;
}
SSD_PNG_HD long long png_stream_bytes(const int H, const int W) { return (long long)H * (1 + 3 * (long long)W); }
SSD_PNG_HD int png_segments(const int H, const int W) { return (int)((png_stream_bytes(H, W) + kPngSeg - 1) / kPngSeg); }
SSD_PNG_HD long long png_bound(const int H, const int W) {
    return 8 + 25 + 12 + (long long)png_segments(H, W) * (12 + 5) + png_stream_bytes(H, W) + 6;
}

// ---- rule 3: tokens ----------------------------------------------------------------------------------------------------
// what the byte at offset `off` of a maximal run of n equal bytes emits: 0 nothing, 1 a literal, else a match of that length
SSD_PNG_HD int png_token(const int off, const int n) {
    if (off == 0) return 1;
    const int k = off - 1, p = k / 258, within = k - p * 258;
    const int left = n - 1 - p * 258, piece = left < 258 ? left : 258;
    if (piece >= 3) return within == 0 ? piece : 0;
    return 1;
}
// a match length 3..258 -> its symbol 257..285 and extra bits
SSD_PNG_HD void png_length_symbol(const int len, int& sym, int& ebits, int& evalue) {
    const int l = len - 3;
    if (len == 258) { sym = 285; ebits = 0; evalue = 0; return; }
    if (l < 8) { sym = 257 + l; ebits = 0; evalue = 0; return; }
    int top = 3;
    while ((l >> (top + 1)) != 0) ++top;
    ebits = top - 2;
    sym = 257 + 4 * ebits + (l >> ebits);
    evalue = l & ((1 << ebits) - 1);
}
SSD_PNG_HD int png_symbol_extra(const int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// ---- bits, least significant first, ORed into 32-bit words that other threads write too -------------------------------
SSD_PNG_HD void png_or(unsigned* word, const unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(word, v);
#else
    *word |= v;
#endif
}
SSD_PNG_HD void png_add(unsigned* word, const unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(word, v);
#else
    *word += v;
#endif
}
SSD_PNG_HD void png_xor(unsigned* word, const unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicXor(word, v);
#else
    *word ^= v;
#endif
}
struct png_bit_sink {
    unsigned* words;
    int at;                     // the word `cur` goes to
    unsigned long long cur;     // `fill` < 32 bits not yet written, from bit 0 up
    int fill;
    SSD_PNG_HD void begin(unsigned* w, const unsigned bit) { words = w; at = (int)(bit >> 5); cur = 0; fill = (int)(bit & 31u); }
    // value < 2^n, n <= 32
    SSD_PNG_HD void put(const unsigned value, const int n) {
        cur |= (unsigned long long)value << fill;
        fill += n;
        if (fill >= 32) {
            png_or(words + at, (unsigned)cur);
            ++at;
            cur >>= 32;
            fill -= 32;
        }
    }
    SSD_PNG_HD void to_byte() { put(0u, (8 - (fill & 7)) & 7); }
    SSD_PNG_HD void finish() { if (fill) png_or(words + at, (unsigned)cur); fill = 0; cur = 0; }
};

// ---- rule 4: the two codes --------------------------------------------------------------------------------------------
struct png_huff_work {
    unsigned freq[2 * kPngLit];             // leaves in ascending order, then the internal nodes in the order they are made
    unsigned short parent[2 * kPngLit];
    unsigned short depth[2 * kPngLit];
    unsigned short count[2 * kPngLit];      // codes per length
};
// what a segment's code building reads and writes; in LDS on the device
struct png_codes {
    unsigned hist[kPngLit + 2];             // literal / length frequencies
    unsigned clhist[kPngCl + 1];
    unsigned short order[kPngLit + 2];      // symbols in ascending (frequency, symbol) order
    unsigned short lcode[kPngLit + 2];      // codes as they go into the stream: bit-reversed
    unsigned short clcode[kPngCl + 1];
    unsigned char llen[kPngLit + 2];
    unsigned char cllen[kPngCl + 1];
    png_huff_work work;
};

// the place of symbol i among freq[0..n) in ascending (frequency, symbol) order
SSD_PNG_HD int png_rank(const unsigned* freq, const int n, const int i) {
    const unsigned f = freq[i];
    int r = 0;
    for (int j = 0; j < n; ++j) r += (freq[j] < f || (freq[j] == f && j < i)) ? 1 : 0;
    return r;
}

// Code lengths of at most `limit` bits for the symbols with a nonzero frequency (`order`: all n symbols, ascending), 0 for
// the others.  Plain Huffman (two queues; of two equal weights the leaf goes first); where its depth exceeds the limit, the
// counts per length are shortened as ITU-T T.81 K.3 does it -- two codes of the longest length become one of the length
// above and a shorter code is split -- which keeps the Kraft sum at exactly 1, and the lengths go out longest first to the
// rarest symbols.  Two used symbols at least.
SSD_PNG_HD void png_huffman(const unsigned* freq, const unsigned short* order, const int n, const int limit, unsigned char* len,
                            png_huff_work& w) {
    int z = 0;
    while (z < n && freq[order[z]] == 0) ++z;
    const int m = n - z;
    for (int i = 0; i < n; ++i) len[i] = 0;
    if (m < 2) {
        if (m == 1) len[order[z]] = 1;
        return;
    }
    for (int k = 0; k < m; ++k) w.freq[k] = freq[order[z + k]];
    int a = 0, b = m;
    for (int next = m; next < 2 * m - 1; ++next) {
        unsigned sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
            int node;
            if (a < m && (b >= next || w.freq[a] <= w.freq[b])) node = a++; else node = b++;
            sum += w.freq[node];
            w.parent[node] = (unsigned short)next;
        }
        w.freq[next] = sum;
    }
    w.depth[2 * m - 2] = 0;
    int deepest = 0;
    for (int k = 2 * m - 3; k >= 0; --k) {
        w.depth[k] = (unsigned short)(w.depth[w.parent[k]] + 1);
        if (k < m && w.depth[k] > deepest) deepest = w.depth[k];
    }
    if (deepest <= limit) {
        for (int k = 0; k < m; ++k) len[order[z + k]] = (unsigned char)w.depth[k];
        return;
    }
    for (int d = 0; d <= deepest; ++d) w.count[d] = 0;
    for (int k = 0; k < m; ++k) ++w.count[w.depth[k]];
    for (int i = deepest; i > limit; --i) {
        while (w.count[i] > 1) {                                                   // the deepest codes come in pairs
            int j = i - 2;
            while (j > 0 && w.count[j] == 0) --j;
            w.count[i] = (unsigned short)(w.count[i] - 2);
            ++w.count[i - 1];
            w.count[j + 1] = (unsigned short)(w.count[j + 1] + 2);
            --w.count[j];
        }
    }
    int k = 0;
    for (int d = limit; d >= 1; --d)
        for (int c = 0; c < w.count[d]; ++c) len[order[z + k++]] = (unsigned char)d;
}

// canonical codes (RFC 1951 3.2.2) of lengths up to 15, bit-reversed: Huffman codes enter the stream most significant bit first
SSD_PNG_HD void png_assign_codes(const unsigned char* len, const int n, unsigned short* code, png_huff_work& w) {
    for (int d = 0; d <= 16; ++d) w.count[d] = 0;
    for (int i = 0; i < n; ++i) ++w.count[len[i]];
    w.count[0] = 0;
    unsigned next = 0;
    w.depth[0] = 0;
    for (int d = 1; d <= 15; ++d) {
        next = (next + w.count[d - 1]) << 1;
        w.depth[d] = (unsigned short)next;                                         // the first code of length d
    }
    for (int i = 0; i < n; ++i) {
        const int d = len[i];
        unsigned r = 0;
        if (d) {
            const unsigned c = w.depth[d]++;
            for (int k = 0; k < d; ++k) r |= ((c >> k) & 1u) << (d - 1 - k);
        }
        code[i] = (unsigned short)r;
    }
}

// The block header's code lengths -- the kPngLit literal / length lengths, then the distance code's 1 -- as code-length
// symbols: a maximal run of z zeros goes out as 18 (11..138 zeros) while 11 or more are left, then 17 for 3..10, single
// zeros for 1 or 2.  Symbol 16 is not used.
template <class Sink>
SSD_PNG_HD void png_length_sequence(const unsigned char* llen, Sink& s) {
    int i = 0;
    while (i < kPngSeq) {
        const int v = i < kPngLit ? llen[i] : 1;
        if (v) { s.symbol(v, 0, 0); ++i; continue; }
        int j = i;
        while (j < kPngLit && llen[j] == 0) ++j;
        int zeros = j - i;
        while (zeros >= 11) {
            const int r = zeros < 138 ? zeros : 138;
            s.symbol(18, 7, r - 11);
            zeros -= r;
        }
        if (zeros >= 3) { s.symbol(17, 3, zeros - 3); zeros = 0; }
        for (; zeros > 0; --zeros) s.symbol(0, 0, 0);
        i = j;
    }
}
struct png_cl_count_sink {
    unsigned* hist;
    unsigned extra;
    SSD_PNG_HD void symbol(const int sym, const int ebits, const int) { ++hist[sym]; extra += (unsigned)ebits; }
};
struct png_cl_write_sink {
    png_bit_sink* bits;
    const unsigned short* code;
    const unsigned char* len;
    SSD_PNG_HD void symbol(const int sym, const int ebits, const int evalue) {
        bits->put(code[sym], len[sym]);
        if (ebits) bits->put((unsigned)evalue, ebits);
    }
};

// ---- a segment ---------------------------------------------------------------------------------------------------------
struct png_segment {
    alignas(16) unsigned char in[kPngSeg + 16];     // the segment's bytes of the filtered stream, zeros behind them
    alignas(16) unsigned out[kPngSlot / 4];         // its finished chunk data, little-endian words, zeros behind it
    int first[kPngThreads], last[kPngThreads];      // where the first / last run of a piece starts (kPngNone / -1: none does)
    unsigned bits[kPngThreads];             // bits of the tokens of a piece
    png_codes c;
    int len;                                // bytes of filtered stream, 1..kPngSeg
    int is_first, is_last;                  // of its image
    unsigned extra_cl;                      // extra bits of the header's code-length symbols
    unsigned header_bits, dynamic, nbytes;  // of the dynamic block; whether it won; bytes of finished chunk data
    unsigned adler_a, adler_b, crc;         // sums over the threads
};

SSD_PNG_HD int png_pieces(const int len) { return (len + kPngPiece - 1) / kPngPiece; }

// phase 0, thread t: what the sums start from (in[] and len, is_first, is_last are set by the caller)
SSD_PNG_HD void png_phase_clear(png_segment& s, const int t) {
    for (int i = t; i < kPngSlot / 4; i += kPngThreads) s.out[i] = 0;
    for (int i = t; i < kPngLit + 2; i += kPngThreads) s.c.hist[i] = 0;
    if (t < kPngCl + 1) s.c.clhist[t] = 0;
    if (t == 0) { s.adler_a = 0; s.adler_b = 0; s.crc = 0; s.extra_cl = 0; }
}

// phase 1: the runs that start in piece t
SSD_PNG_HD void png_phase_bounds(png_segment& s, const int t) {
    const int lo = t * kPngPiece, hi = lo + kPngPiece < s.len ? lo + kPngPiece : s.len;
    int first = kPngNone, last = -1;
    for (int i = lo; i < hi; ++i) {
        if (i == 0 || s.in[i] != s.in[i - 1]) {
            if (last < 0) first = i;
            last = i;
        }
    }
    s.first[t] = first;
    s.last[t] = last;
}

// the tokens of piece t, in order: a byte's token follows from where its run starts and ends (rule 3), and a run that
// reaches into the piece started at the last start of an earlier piece and ends at the first start of a later one
template <class Sink>
SSD_PNG_HD void png_walk(const png_segment& s, const int t, Sink& sink) {
    const int lo = t * kPngPiece, hi = lo + kPngPiece < s.len ? lo + kPngPiece : s.len;
    if (lo >= hi) return;
    int start = 0, end = s.len;
    for (int u = t - 1; u >= 0; --u)
        if (s.last[u] >= 0) { start = s.last[u]; break; }
    const int pieces = png_pieces(s.len);
    for (int u = t + 1; u < pieces; ++u)
        if (s.first[u] != kPngNone) { end = s.first[u]; break; }
    int i = lo;
    while (i < hi) {
        if (i == 0 || s.in[i] != s.in[i - 1]) start = i;
        int j = i + 1;
        while (j < hi && s.in[j] == s.in[j - 1]) ++j;
        const int n = (j < hi ? j : end) - start;
        const int value = s.in[i];
        for (int k = i; k < j; ++k) {
            const int token = png_token(k - start, n);
            if (token == 1) sink.literal(value);
            else if (token) sink.match(token);
        }
        i = j;
    }
}
struct png_hist_sink {
    unsigned* hist;
    SSD_PNG_HD void literal(const int v) { png_add(hist + v, 1u); }
    SSD_PNG_HD void match(const int len) {
        int sym, ebits, evalue;
        png_length_symbol(len, sym, ebits, evalue);
        png_add(hist + sym, 1u);
    }
};
struct png_count_sink {
    const unsigned char* llen;
    unsigned bits;
    SSD_PNG_HD void literal(const int v) { bits += llen[v]; }
    SSD_PNG_HD void match(const int len) {
        int sym, ebits, evalue;
        png_length_symbol(len, sym, ebits, evalue);
        bits += (unsigned)(llen[sym] + ebits + 1);
    }
};
struct png_write_sink {
    png_bit_sink bits;
    const unsigned short* lcode;
    const unsigned char* llen;
    SSD_PNG_HD void literal(const int v) { bits.put(lcode[v], llen[v]); }
    // the length's code, its extra bits, then distance code 0: one 0 bit, no extra bits (distance 1)
    SSD_PNG_HD void match(const int len) {
        int sym, ebits, evalue;
        png_length_symbol(len, sym, ebits, evalue);
        bits.put(lcode[sym], llen[sym]);
        bits.put((unsigned)evalue, ebits + 1);
    }
};

// phase 2: the histogram of the tokens (thread 0 adds the end-of-block symbol) and the Adler-32 sums of the piece:
// a = the sum of the bytes, b = the sum of (len - i) * byte i, both below 2^32 and reduced before they are added up
SSD_PNG_HD void png_phase_hist(png_segment& s, const int t) {
    png_hist_sink sink = {s.c.hist};
    png_walk(s, t, sink);
    if (t == 0) png_add(s.c.hist + 256, 1u);
    const int lo = t * kPngPiece, hi = lo + kPngPiece < s.len ? lo + kPngPiece : s.len;
    unsigned a = 0, b = 0;
    for (int i = lo; i < hi; ++i) { a += s.in[i]; b += (unsigned)(s.len - i) * s.in[i]; }
    if (lo < hi) { png_add(&s.adler_a, a); png_add(&s.adler_b, b % kPngAdlerMod); }
}

// phase 3 (threads i < kPngLit, two per thread) and phase 5 (i < kPngCl): sort the symbols
SSD_PNG_HD void png_phase_rank_lit(png_segment& s, const int t) {
    for (int i = t; i < kPngLit; i += kPngThreads) s.c.order[png_rank(s.c.hist, kPngLit, i)] = (unsigned short)i;
}
SSD_PNG_HD void png_phase_rank_cl(png_segment& s, const int t) {
    if (t < kPngCl) s.c.order[png_rank(s.c.clhist, kPngCl, t)] = (unsigned short)t;
}

// phase 4, thread 0: the literal / length code and what its lengths cost as code-length symbols
SSD_PNG_HD void png_phase_plan_lit(png_segment& s, const int t) {
    if (t != 0) return;
    png_huffman(s.c.hist, s.c.order, kPngLit, 15, s.c.llen, s.c.work);
    png_cl_count_sink sink = {s.c.clhist, 0u};
    png_length_sequence(s.c.llen, sink);
    s.extra_cl = sink.extra;
}

// phase 6, thread 0: the code-length code, both codes' bits, the sizes, the choice, and the block's front
SSD_PNG_HD void png_phase_plan_block(png_segment& s, const int t) {
    if (t != 0) return;
    png_codes& c = s.c;
    png_huffman(c.clhist, c.order, kPngCl, 7, c.cllen, c.work);
    png_assign_codes(c.llen, kPngLit, c.lcode, c.work);
    png_assign_codes(c.cllen, kPngCl, c.clcode, c.work);
    unsigned header = 3 + 5 + 5 + 4 + 3 * kPngCl + s.extra_cl, data = 0;
    for (int i = 0; i < kPngCl; ++i) header += c.clhist[i] * c.cllen[i];
    for (int i = 0; i < kPngLit; ++i) data += c.hist[i] * (unsigned)(c.llen[i] + png_symbol_extra(i) + (i > 256 ? 1 : 0));
    const unsigned base = s.is_first ? 2u : 0u, bits = header + data;
    // a dynamic block that is not the image's last is followed by an empty stored block: 000, zeros to the byte, 00 00 FF FF
    const unsigned dynamic_bytes = s.is_last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4, stored_bytes = 5u + (unsigned)s.len;
    s.dynamic = dynamic_bytes < stored_bytes ? 1u : 0u;
    s.header_bits = 8 * base + header;
    s.nbytes = base + (s.dynamic ? dynamic_bytes : stored_bytes);
    png_bit_sink w;
    w.begin(s.out, 0u);
    if (s.is_first) { w.put(0x78u, 8); w.put(0x9Cu, 8); }
    w.put(s.is_last ? 1u : 0u, 1);
    if (!s.dynamic) {
        w.put(0u, 2);
        w.to_byte();
        w.put((unsigned)s.len, 16);
        w.put(~(unsigned)s.len & 0xFFFFu, 16);
        w.finish();
        return;
    }
    w.put(2u, 2);
    w.put(kPngLit - 257, 5);
    w.put(0u, 5);
    w.put(kPngCl - 4, 4);
    const unsigned char order[kPngCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < kPngCl; ++i) w.put(c.cllen[order[i]], 3);
    png_cl_write_sink sink = {&w, c.clcode, c.cllen};
    png_length_sequence(c.llen, sink);
    w.finish();
}

// phase 7: the bits of piece t's tokens
SSD_PNG_HD void png_phase_count(png_segment& s, const int t) {
    png_count_sink sink = {s.c.llen, 0u};
    if (s.dynamic) png_walk(s, t, sink);
    s.bits[t] = sink.bits;
}

// phase 8: the tokens' codes behind those of the pieces before (thread 0 also closes the block), or the bytes themselves
SSD_PNG_HD void png_phase_write(png_segment& s, const int t) {
    const int lo = t * kPngPiece, hi = lo + kPngPiece < s.len ? lo + kPngPiece : s.len;
    if (!s.dynamic) {
        if (lo >= hi) return;
        png_bit_sink w;
        w.begin(s.out, 8u * ((s.is_first ? 2u : 0u) + 5u + (unsigned)lo));
        for (int i = lo; i < hi; ++i) w.put(s.in[i], 8);
        w.finish();
        return;
    }
    unsigned before = s.header_bits;
    for (int u = 0; u < t; ++u) before += s.bits[u];
    png_write_sink sink;
    sink.bits.begin(s.out, before);
    sink.lcode = s.c.lcode;
    sink.llen = s.c.llen;
    png_walk(s, t, sink);
    sink.bits.finish();
    if (t != 0) return;
    unsigned end = s.header_bits;
    for (int u = 0; u < kPngThreads; ++u) end += s.bits[u];
    png_bit_sink w;
    w.begin(s.out, end);
    w.put(s.c.lcode[256], s.c.llen[256]);
    if (!s.is_last) {
        w.put(0u, 3);
        w.to_byte();
        w.put(0u, 16);
        w.put(0xFFFFu, 16);
    }
    w.finish();
}

// ---- CRC-32 ------------------------------------------------------------------------------------------------------------
// the register after one more byte (no final inversion)
SSD_PNG_HD unsigned png_crc_byte(unsigned crc, const unsigned byte) {
    crc ^= byte;
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ ((crc & 1u) ? kPngCrcPoly : 0u);
    return crc;
}
// a * b modulo the CRC polynomial, bit-reflected
SSD_PNG_HD unsigned png_gf2_mul(const unsigned a, unsigned b) {
    unsigned p = 0;
    for (unsigned m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kPngCrcPoly : b >> 1;
    }
    return p;
}
// x^(2^k) modulo the polynomial, k = 0..31: constants, made once on the host and handed to the kernels by value
struct png_crc_powers { unsigned x2n[32]; };
static inline png_crc_powers png_crc_build_powers() {
    png_crc_powers p;
    p.x2n[0] = 1u << 30;
    for (int k = 1; k < 32; ++k) p.x2n[k] = png_gf2_mul(p.x2n[k - 1], p.x2n[k - 1]);
    return p;
}
// the register `crc` after n more zero bytes, as a linear map: crc * x^(8 n)
SSD_PNG_HD unsigned png_crc_shift(const unsigned crc, const unsigned n, const unsigned* x2n) {
    unsigned p = crc;
    for (unsigned e = 8u * n, k = 0; e; e >>= 1, ++k)
        if (e & 1u) p = png_gf2_mul(x2n[k], p);
    return p;
}
// phase 9: the CRC register (from zero) of piece t of the finished data, moved behind the data's last byte; the register is
// linear in (start value, data), so the XOR of the pieces is the register of the whole data from zero
SSD_PNG_HD void png_phase_crc(png_segment& s, const int t, const unsigned* x2n) {
    const int n = (int)s.nbytes, lo = t * kPngCrcPiece, hi = lo + kPngCrcPiece < n ? lo + kPngCrcPiece : n;
    if (lo >= hi) return;
    unsigned crc = 0;
    for (int i = lo; i < hi; ++i) crc = png_crc_byte(crc, (s.out[i >> 2] >> (8 * (i & 3))) & 255u);
    png_xor(&s.crc, png_crc_shift(crc, (unsigned)(n - hi), x2n));
}
// the register after "IDAT" and the segment's data, from the sum of phase 9
SSD_PNG_HD unsigned png_chunk_crc_register(const png_segment& s, const unsigned* x2n) {
    unsigned head = 0xFFFFFFFFu;
    head = png_crc_byte(head, 'I'); head = png_crc_byte(head, 'D'); head = png_crc_byte(head, 'A'); head = png_crc_byte(head, 'T');
    return png_crc_shift(head, s.nbytes, x2n) ^ s.crc;
}

// ---- Adler-32 ----------------------------------------------------------------------------------------------------------
// (A, B) of a stream followed by a segment of `len` bytes with sums (a, b) as phase 2 makes them
SSD_PNG_HD void png_adler_append(unsigned& A, unsigned& B, const unsigned a, const unsigned b, const unsigned len) {
    B = (B + (len * A) % kPngAdlerMod + b % kPngAdlerMod) % kPngAdlerMod;
    A = (A + a % kPngAdlerMod) % kPngAdlerMod;
}

SSD_PNG_HD void png_put_be32(unsigned char* at, const unsigned v) {
    at[0] = (unsigned char)(v >> 24); at[1] = (unsigned char)(v >> 16); at[2] = (unsigned char)(v >> 8); at[3] = (unsigned char)v;
}
// the signature and IHDR of a W x H, 8-bit RGB, non-interlaced image
SSD_PNG_HD void png_front(unsigned char* at, const int H, const int W) {
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) at[i] = sig[i];
    png_put_be32(at + 8, 13u);
    at[12] = 'I'; at[13] = 'H'; at[14] = 'D'; at[15] = 'R';
    png_put_be32(at + 16, (unsigned)W);
    png_put_be32(at + 20, (unsigned)H);
    at[24] = 8; at[25] = 2; at[26] = 0; at[27] = 0; at[28] = 0;
    unsigned crc = 0xFFFFFFFFu;
    for (int i = 12; i < 29; ++i) crc = png_crc_byte(crc, at[i]);
    png_put_be32(at + 29, ~crc);
}
SSD_PNG_HD void png_iend(unsigned char* at) {
    const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) at[i] = iend[i];
}

// ---- the decoder (ssd_png_dec.hip): the format contract of include/ssd_hip.h, "PNG DECODER" ----------------------------
// the inverse of png_filter, for any filter distance: x is the filtered byte, a / b / c the raw bytes to the left, above and
// above-left (0 outside the image)
SSD_PNG_HD unsigned png_unfilter(const int type, const int x, const int a, const int b, const int c) {
    const int pred = type == 0 ? 0 : (type == 1 ? a : (type == 2 ? b : (type == 3 ? (a + b) >> 1 : png_paeth(a, b, c))));
    return (unsigned)(x + pred) & 255u;
}
SSD_PNG_HD int png_channels(const int color_type) { return color_type == 2 ? 3 : (color_type == 6 ? 4 : (color_type == 4 ? 2 : 1)); }
// the (colour type, depth) pairs the decoder takes: every pair of the PNG specification but grey at 16 bits
SSD_PNG_HD bool png_format_ok(const int color_type, const int depth) {
    if (color_type == 0 || color_type == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    if (color_type == 2 || color_type == 4 || color_type == 6) return depth == 8 || depth == 16;
    return false;
}
SSD_PNG_HD long long png_row_bytes(const int W, const int color_type, const int depth) {
    return ((long long)W * png_channels(color_type) * depth + 7) >> 3;
}
SSD_PNG_HD int png_filter_distance(const int color_type, const int depth) {
    const int v = png_channels(color_type) * depth / 8;
    return v < 1 ? 1 : v;
}
// pixel x of an unfiltered row -> R, G, B: sub-byte samples unpacked (grey scaled to 0..255), the palette looked up (768
// bytes, zeros behind the file's entries), grey replicated, alpha dropped, the high byte of a 16-bit sample
SSD_PNG_HD void png_pixel_rgb(const unsigned char* row, const int x, const int color_type, const int depth, const unsigned char* palette,
                              unsigned char* rgb) {
    if (depth < 8) {
        const int bit = x * depth;
        const int s = (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
        if (color_type == 3) {
            rgb[0] = palette[3 * s]; rgb[1] = palette[3 * s + 1]; rgb[2] = palette[3 * s + 2];
        } else {
            rgb[0] = rgb[1] = rgb[2] = (unsigned char)(s * (255 / ((1 << depth) - 1)));
        }
        return;
    }
    const int step = depth >> 3;
    const unsigned char* p = row + (long long)x * png_channels(color_type) * step;
    if (color_type == 3) {
        const int s = p[0];
        rgb[0] = palette[3 * s]; rgb[1] = palette[3 * s + 1]; rgb[2] = palette[3 * s + 2];
    } else if (color_type == 2 || color_type == 6) {
        rgb[0] = p[0]; rgb[1] = p[step]; rgb[2] = p[2 * step];
    } else {
        rgb[0] = rgb[1] = rgb[2] = p[0];
    }
}

}  // namespace ssd
