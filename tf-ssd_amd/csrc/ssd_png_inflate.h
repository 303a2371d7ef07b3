// What the device inflater's kernel and its host model (both in ssd_png_inflate.hip) share: RFC 1950 / 1951 decoding as step
// functions (include/ssd_hip.h, "PNG INFLATE"; DESIGN.md section 7, "PNG inflate on the device").  A stream is decoded by
// LANES "lanes" that hold the same decode state (bit buffer, position, status: wave-uniform on the device) and share one
// png_inf_work; only four things are divided among them: building a block's code tables, copying a match or a stored
// block into the window, writing a finished half of the window out, and folding it into the Adler-32.  Each of those is a
// phase that reads only what earlier phases wrote, with a barrier behind it, so the kernel runs it on 64 lanes and the host
// model runs it with LANES = 1 as a plain loop; what lanes share is summed (integer, commutative).  The bytes and the status
// word therefore do not depend on LANES.  Integer arithmetic only.
#pragma once
#include "ssd_png_common.h"

namespace ssd {

enum : int {
    kInfWindow = 32768,         // the ring: deflate's largest distance
    kInfHalf = 16384,           // what is written out (and folded into the Adler-32) at a time
    kInfStage = 4096,           // bytes of input staged at a time (+ 16 of slack)
    kInfLitFast = 10,           // bits the literal / length code's direct table resolves; longer codes walk the counts
    kInfDistFast = 8,           // the same for the distance code and the code-length code
    kInfPiece = 256,            // bytes of a half one lane folds into the Adler-32 at a time
    kInfLens = 320,             // 288 literal / length + 32 distance code lengths
};
static const long long kInfMaxStream = SSD_PNG_INFLATE_MAX_STREAM;    // the cap on H * (1 + row_bytes): include/ssd_hip.h has the reasoning

// SSD_PNG_INF_SAME(x): a 32-bit value every lane holds alike (read from LDS at a wave-uniform address), handed to the
// scalar unit, so the decode state that follows from it (bit buffer, position, branches) stays out of the vector registers
#if defined(__HIP_DEVICE_COMPILE__)
#define SSD_PNG_INF_SYNC() __syncthreads()
#define SSD_PNG_INF_SAME(x) ((unsigned)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define SSD_PNG_INF_SYNC() ((void)0)
#define SSD_PNG_INF_SAME(x) ((unsigned)(x))
#endif

struct png_inf_code {
    unsigned count[16];             // codes of each length
    unsigned short offs[16];        // where a length's symbols begin in `sorted`
    unsigned short sorted[288];     // the symbols by (length, symbol): canonical order
};
struct png_inf_work {
    alignas(16) unsigned char window[kInfWindow];
    alignas(16) unsigned stage[kInfStage / 4 + 4];
    png_inf_code lit, dist;         // `dist` holds the code-length code while a dynamic header is read
    unsigned short lit_fast[1 << kInfLitFast], dist_fast[1 << kInfDistFast];   // (symbol << 4) | length; 0: walk
    unsigned char lens[kInfLens], cl[20];
    unsigned acc[2];                // what the lanes add up for the Adler-32 of one flush
};
struct png_inf_bits {
    const unsigned char* in;
    long long n, pos, base;         // bytes of input; bytes taken into `hold`; the input offset stage[0] holds
    unsigned long long hold;        // `nbits` bits not yet used, from bit 0 up
    int nbits;
    SSD_PNG_HD unsigned take(const int k) {     // k <= 32 <= nbits
        const unsigned v = (unsigned)(hold & ((1ull << k) - 1ull));
        hold >>= k;
        nbits -= k;
        return v;
    }
    // more bits used than the input has: what was read past its end were zeros
    SSD_PNG_HD bool over() const { return 8 * pos - nbits > 8 * n; }
};

SSD_PNG_HD void png_inf_copy16(unsigned char* dst, const unsigned char* src) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
#else
    for (int i = 0; i < 16; ++i) dst[i] = src[i];
#endif
}

// kInfStage + 16 bytes of input from `at` (rounded down to 16) on, zeros behind the input's end; no byte outside [0, n) is read
template <int LANES>
SSD_PNG_HD void png_inf_stage(png_inf_work& w, png_inf_bits& s, const long long at, const int lane) {
    SSD_PNG_INF_SYNC();
    s.base = at & ~15ll;
    unsigned char* stage = reinterpret_cast<unsigned char*>(w.stage);
    for (int g = lane; g < kInfStage / 16 + 1; g += LANES) {
        const long long o = s.base + 16ll * g;
        if (o + 16 <= s.n) {
            png_inf_copy16(stage + 16 * g, s.in + o);
        } else {
            for (int k = 0; k < 4; ++k) {
                unsigned v = 0;
                for (int j = 0; j < 4; ++j)
                    if (o + 4 * k + j < s.n) v |= (unsigned)s.in[o + 4 * k + j] << (8 * j);
                w.stage[4 * g + k] = v;
            }
        }
    }
    SSD_PNG_INF_SYNC();
}

// at least 32 bits in `hold` behind this
template <int LANES>
SSD_PNG_HD void png_inf_refill(png_inf_work& w, png_inf_bits& s, const int lane) {
    if (s.nbits >= 32) return;
    if (s.pos < s.base || s.pos + 4 > s.base + kInfStage + 12) png_inf_stage<LANES>(w, s, s.pos, lane);
    const int off = (int)(s.pos - s.base);
    const unsigned long long two = ((unsigned long long)SSD_PNG_INF_SAME(w.stage[(off >> 2) + 1]) << 32) | SSD_PNG_INF_SAME(w.stage[off >> 2]);
    s.hold |= (unsigned long long)(unsigned)(two >> (8 * (off & 3))) << s.nbits;
    s.nbits += 32;
    s.pos += 4;
}

// the symbol whose code the low bits of `bits` begin with (first bit = the code's most significant), codes up to `maxlen`
// bits; SAME: every lane asks with the same bits
template <bool SAME>
SSD_PNG_HD int png_inf_walk(const png_inf_code& c, unsigned bits, const int maxlen, int& len_out) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= maxlen; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int cnt = (int)SSD_PNG_INF_SAME(c.count[len]);
        if (code - cnt < first) {
            len_out = len;
            return SAME ? (int)SSD_PNG_INF_SAME(c.sorted[index + (code - first)]) : (int)c.sorted[index + (code - first)];
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

// the next symbol, or -1 (a code of an incomplete set that no symbol has): nothing is dropped then
SSD_PNG_HD int png_inf_decode(const png_inf_code& c, const unsigned short* fast, const int fastbits, png_inf_bits& s) {
    const unsigned e = SSD_PNG_INF_SAME(fast[(unsigned)s.hold & ((1u << fastbits) - 1u)]);
    if (e) {
        s.take((int)(e & 15u));
        return (int)(e >> 4);
    }
    int len = 0;
    const int sym = png_inf_walk<true>(c, (unsigned)s.hold, 15, len);
    if (sym >= 0) s.take(len);
    return sym;
}

// One code's tables from its n lengths.  kind 0: the code-length code, 1: literal / length, 2: distance.  An incomplete set
// passes only as zlib lets it: a single code of one bit (kinds 1 and 2), or no code at all (kind 2).
template <int LANES>
SSD_PNG_HD unsigned png_inf_build(png_inf_code& c, unsigned short* fast, const int fastbits, const unsigned char* lens, const int n, const int kind,
                                  const int lane) {
    for (int i = lane; i < 16; i += LANES) c.count[i] = 0;
    SSD_PNG_INF_SYNC();
    for (int s = lane; s < n; s += LANES) png_add(&c.count[lens[s]], 1u);
    SSD_PNG_INF_SYNC();
    int left = 1, total = 0;
    for (int len = 1; len <= 15; ++len) {
        const int cnt = (int)SSD_PNG_INF_SAME(c.count[len]);
        left = (left << 1) - cnt;
        if (left < 0) return SSD_PNG_INFLATE_OVERSUBSCRIBED;
        if (lane == 0) c.offs[len] = (unsigned short)total;
        total += cnt;
    }
    if (left > 0 && !((kind != 0 && total == 1 && SSD_PNG_INF_SAME(c.count[1]) == 1) || (kind == 2 && total == 0))) return SSD_PNG_INFLATE_INCOMPLETE;
    SSD_PNG_INF_SYNC();
    for (int len = 1 + lane; len <= 15; len += LANES) {
        int o = c.offs[len];
        for (int s = 0; s < n; ++s)
            if (lens[s] == len) c.sorted[o++] = (unsigned short)s;
    }
    SSD_PNG_INF_SYNC();
    for (int e = lane; e < (1 << fastbits); e += LANES) {
        int len = 0;
        const int sym = png_inf_walk<false>(c, (unsigned)e, fastbits, len);
        fast[e] = sym >= 0 ? (unsigned short)((sym << 4) | len) : (unsigned short)0;
    }
    SSD_PNG_INF_SYNC();
    return 0;
}

// Bytes [done, done + m) of the output leave the ring (done: a multiple of kInfHalf; m <= kInfHalf) and enter the Adler-32.
template <int LANES>
SSD_PNG_HD void png_inf_flush(png_inf_work& w, unsigned char* out, const long long done, const int m, unsigned& A, unsigned& B, const int lane) {
    const unsigned char* src = w.window + (done & (kInfWindow - 1));
    if (lane == 0) w.acc[0] = w.acc[1] = 0;
    SSD_PNG_INF_SYNC();                                      // and every write to the half has landed
    for (int i = 16 * lane; i + 16 <= m; i += 16 * LANES) png_inf_copy16(out + done + i, src + i);
    for (int i = (m & ~15) + lane; i < m; i += LANES) out[done + i] = src[i];
    const int pieces = (m + kInfPiece - 1) / kInfPiece;
    for (int pc = lane; pc < pieces; pc += LANES) {
        const int s0 = pc * kInfPiece, e0 = s0 + kInfPiece < m ? s0 + kInfPiece : m;
        unsigned a = 0, b = 0;                              // b: every byte times its distance to the piece's end
        for (int j = s0; j < e0; ++j) {
            a += src[j];
            b += a;
        }
        png_add(&w.acc[0], a);
        png_add(&w.acc[1], (b + a * (unsigned)(m - e0)) % kPngAdlerMod);
    }
    SSD_PNG_INF_SYNC();
    B = (B + (unsigned)m * A + SSD_PNG_INF_SAME(w.acc[1])) % kPngAdlerMod;
    A = (A + SSD_PNG_INF_SAME(w.acc[0])) % kPngAdlerMod;
    SSD_PNG_INF_SYNC();
}

// One zlib stream of n bytes -> at most n_out bytes at `out`; the status word (0: exactly n_out bytes, zlib's).  Every loop
// consumes input bits or produces owed output; a byte past n_out is never written.
template <int LANES>
SSD_PNG_HD unsigned png_inflate_stream(png_inf_work& w, const unsigned char* in, const long long n, unsigned char* out, const long long n_out,
                                       const int lane) {
    png_inf_bits s;
    s.in = in; s.n = n; s.pos = 0; s.base = -2ll * kInfStage; s.hold = 0; s.nbits = 0;
    unsigned A = 1, B = 0;
    long long p = 0, done = 0;                              // bytes produced; bytes written out
    png_inf_refill<LANES>(w, s, lane);
    const unsigned cmf = s.take(8), flg = s.take(8);
    if (s.over()) return SSD_PNG_INFLATE_INPUT;
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return SSD_PNG_INFLATE_HEADER;
    const long long dmax = 1ll << ((cmf >> 4) + 8);
    unsigned last = 0;
    do {
        png_inf_refill<LANES>(w, s, lane);
        last = s.take(1);
        const unsigned type = s.take(2);
        if (s.over()) return SSD_PNG_INFLATE_INPUT;
        if (type == 3) return SSD_PNG_INFLATE_BLOCK_TYPE;
        if (type == 0) {
            s.take(s.nbits & 7);
            png_inf_refill<LANES>(w, s, lane);
            const unsigned len = s.take(16), nlen = s.take(16);
            if (s.over()) return SSD_PNG_INFLATE_INPUT;
            if (len != (~nlen & 0xFFFFu)) return SSD_PNG_INFLATE_STORED;
            s.pos -= s.nbits >> 3;                          // whole bytes: back to the input
            s.hold = 0;
            s.nbits = 0;
            if (s.pos + len > n) return SSD_PNG_INFLATE_INPUT;
            if (p + len > n_out) return SSD_PNG_INFLATE_OUTPUT;
            int left = (int)len;
            while (left > 0) {
                const int room = kInfHalf - (int)(p - done), step = left < room ? left : room;
                for (int i = lane; i < step; i += LANES) w.window[(p + i) & (kInfWindow - 1)] = in[s.pos + i];
                p += step;
                s.pos += step;
                left -= step;
                if (p - done >= kInfHalf) {
                    png_inf_flush<LANES>(w, out, done, kInfHalf, A, B, lane);
                    done += kInfHalf;
                }
            }
            continue;
        }
        if (type == 1) {
            for (int i = lane; i < kInfLens; i += LANES) w.lens[i] = (unsigned char)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : (i < 288 ? 8 : 5))));
            SSD_PNG_INF_SYNC();
            png_inf_build<LANES>(w.lit, w.lit_fast, kInfLitFast, w.lens, 288, 1, lane);
            png_inf_build<LANES>(w.dist, w.dist_fast, kInfDistFast, w.lens + 288, 32, 2, lane);
        } else {
            const unsigned hlit = s.take(5) + 257, hdist = s.take(5) + 1, hclen = s.take(4) + 4;
            if (s.over()) return SSD_PNG_INFLATE_INPUT;
            if (hlit > 286 || hdist > 30) return SSD_PNG_INFLATE_SYMBOLS;
            for (int i = lane; i < 19; i += LANES) w.cl[i] = 0;
            SSD_PNG_INF_SYNC();
            for (unsigned i = 0; i < hclen; ++i) {
                png_inf_refill<LANES>(w, s, lane);
                const unsigned v = s.take(3);
                // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                const int at = i < 3 ? 16 + (int)i : (i == 3 ? 0 : ((i & 1) ? (int)((19 - i) >> 1) : 6 + (int)(i >> 1)));
                if (lane == 0) w.cl[at] = (unsigned char)v;
            }
            if (s.over()) return SSD_PNG_INFLATE_INPUT;
            SSD_PNG_INF_SYNC();
            unsigned st = png_inf_build<LANES>(w.dist, w.dist_fast, kInfDistFast, w.cl, 19, 0, lane);
            if (st) return st;
            const int total = (int)(hlit + hdist);
            int at = 0, prev = 0;
            while (at < total) {
                png_inf_refill<LANES>(w, s, lane);
                const int sym = png_inf_decode(w.dist, w.dist_fast, kInfDistFast, s);
                if (s.over()) return SSD_PNG_INFLATE_INPUT;
                if (sym < 0) return SSD_PNG_INFLATE_SYMBOL;
                if (sym < 16) {
                    if (lane == 0) w.lens[at] = (unsigned char)sym;
                    prev = sym;
                    ++at;
                    continue;
                }
                if (sym == 16 && at == 0) return SSD_PNG_INFLATE_REPEAT;
                const int rep = sym == 16 ? 3 + (int)s.take(2) : (sym == 17 ? 3 + (int)s.take(3) : 11 + (int)s.take(7));
                if (s.over()) return SSD_PNG_INFLATE_INPUT;
                if (at + rep > total) return SSD_PNG_INFLATE_REPEAT;
                if (sym != 16) prev = 0;
                for (int i = lane; i < rep; i += LANES) w.lens[at + i] = (unsigned char)prev;
                at += rep;
            }
            SSD_PNG_INF_SYNC();
            if (SSD_PNG_INF_SAME(w.lens[256]) == 0) return SSD_PNG_INFLATE_NO_END;
            st = png_inf_build<LANES>(w.lit, w.lit_fast, kInfLitFast, w.lens, (int)hlit, 1, lane);
            if (st) return st;
            st = png_inf_build<LANES>(w.dist, w.dist_fast, kInfDistFast, w.lens + hlit, (int)hdist, 2, lane);
            if (st) return st;
        }
        for (;;) {
            png_inf_refill<LANES>(w, s, lane);
            const int sym = png_inf_decode(w.lit, w.lit_fast, kInfLitFast, s);
            if (s.over()) return SSD_PNG_INFLATE_INPUT;
            if (sym < 0 || sym >= 286) return SSD_PNG_INFLATE_SYMBOL;
            if (sym == 256) break;
            if (sym < 256) {
                if (p >= n_out) return SSD_PNG_INFLATE_OUTPUT;
                if (lane == 0) w.window[p & (kInfWindow - 1)] = (unsigned char)sym;
                ++p;
            } else {
                const int le = sym < 261 || sym == 285 ? 0 : (sym - 261) >> 2;
                const int len = sym == 285 ? 258 : (sym < 261 ? sym - 254 : 3 + ((4 + ((sym - 261) & 3)) << le) + (int)s.take(le));
                png_inf_refill<LANES>(w, s, lane);
                const int dsym = png_inf_decode(w.dist, w.dist_fast, kInfDistFast, s);
                if (s.over()) return SSD_PNG_INFLATE_INPUT;
                if (dsym < 0 || dsym >= 30) return SSD_PNG_INFLATE_SYMBOL;
                const int de = dsym < 4 ? 0 : (dsym >> 1) - 1;
                const long long D = dsym < 4 ? dsym + 1 : 1 + ((2 + (dsym & 1)) << de) + (int)s.take(de);
                if (s.over()) return SSD_PNG_INFLATE_INPUT;
                if (D > p || D > dmax) return SSD_PNG_INFLATE_DISTANCE;
                if (p + len > n_out) return SSD_PNG_INFLATE_OUTPUT;
                // lanes read bytes from before p only (other lanes wrote them: the barrier); a ring slot is read before the
                // same step's write to it
                SSD_PNG_INF_SYNC();
                const long long from = p - D;
                if (D >= len) {
                    for (int l = lane; l < len; l += LANES) w.window[(p + l) & (kInfWindow - 1)] = w.window[(from + l) & (kInfWindow - 1)];
                } else {
                    const int d = (int)D;
                    for (int l = lane; l < len; l += LANES) w.window[(p + l) & (kInfWindow - 1)] = w.window[(from + l % d) & (kInfWindow - 1)];
                }
                p += len;
            }
            if (p - done >= kInfHalf) {
                png_inf_flush<LANES>(w, out, done, kInfHalf, A, B, lane);
                done += kInfHalf;
            }
        }
    } while (!last);
    if (p > done) png_inf_flush<LANES>(w, out, done, (int)(p - done), A, B, lane);
    if (p != n_out) return SSD_PNG_INFLATE_OUTPUT;
    s.take(s.nbits & 7);
    png_inf_refill<LANES>(w, s, lane);
    const unsigned t = s.take(32);
    if (s.over()) return SSD_PNG_INFLATE_INPUT;
    if (((t & 255u) << 24 | (t >> 8 & 255u) << 16 | (t >> 16 & 255u) << 8 | t >> 24) != (B << 16 | A)) return SSD_PNG_INFLATE_ADLER;
    if (s.pos - (s.nbits >> 3) != n) return SSD_PNG_INFLATE_TRAILING;
    return 0;
}

}  // namespace ssd
