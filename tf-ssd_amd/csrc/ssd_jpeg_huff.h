// Huffman DEcoding of a baseline scan as a fixed-point iteration over fixed-size subsequences ("JPEG
// decoding: what runs where").  JPEG Huffman streams self-synchronise: a decoder started at a wrong bit falls into step
// with the true one after a few dozen codes.  So a segment (one restart interval, or the whole scan) is cut into
// subsequences of `subseq_bits` bits, every subsequence but the first starts from the guess "a DC code of MCU block 0
// begins at my first bit", and the entry states are swept until none changes; the first subsequence's state is known, so
// the fixed point is the true decode -- exact, not heuristic.  This header holds what one "thread" does in each phase, as
// __host__ __device__ functions: the kernels (ssd_jpeg_unpack.hip) and the host model (ssd_jpeg_entropy_decode_subseq in
// ssd_jpeg.hip) run the same code, so the algorithm is testable, and checkable under sanitizers, without a GPU.
//
// Bit positions count the STUFFED bytes of the segment: p = 8 * byte + bit.  The 0x00 after an 0xFF holds no data and is
// stepped over; inside a segment every 0xFF is a data byte followed by such a 0x00 (the segment ends before the first 0xFF
// that is not), so "byte i is stuffing" is the local test data[i] == 0 && data[i - 1] == 0xFF.
#pragma once
#include "ssd_jpeg_common.h"

namespace ssd {

static const int kUnpackChunk = 256;            // subsequences a workgroup sweeps at a time; also the cap on sweeps
static const int kUnpackDefaultBits = SSD_JPEG_UNPACK_SUBSEQ_BITS;

// flags of status_dev / of the host model's refusal
enum : int {
    kUnpackBadCode = 1,         // a code outside its table, or a coefficient index past 63
    kUnpackShort = 2,           // the bits ran out before the segment's last MCU
    kUnpackEarly = 4,           // a restart interval whose last code does not end inside the segment's last byte
    kUnpackTables = 8,          // segment tables or states no plan produces (device memory the host cannot check)
};

struct huff_view {
    const unsigned short* look;
    const int* maxcode;
    const int* valoff;
    const unsigned char* vals;
};
__host__ __device__ __forceinline__ huff_view huff_view_of(const ssd_jpeg_huff* t) {
    huff_view v = {t->look, t->maxcode, t->valoff, t->vals};
    return v;
}

struct unpack_seg {
    const unsigned char* data;  // the segment's first byte
    unsigned len;               // its stuffed bytes; 8 * len < 2^31
};

struct unpack_state {
    unsigned p;                 // bit position of the next code
    int z, k;                   // block within the MCU; zigzag index, 0: a DC code comes next
};
__host__ __device__ __forceinline__ bool operator!=(const unpack_state& a, const unpack_state& b) {
    return a.p != b.p || a.z != b.z || a.k != b.k;
}

// what follows from the frame: luma blocks per MCU, blocks per MCU, MCUs
struct unpack_frame {
    jpeg_geometry g;
    int hs, vs, nl, nz, mcus;
};
__host__ __device__ __forceinline__ unpack_frame unpack_frame_of(const int H, const int W, const int hs, const int vs, const int components) {
    unpack_frame f;
    f.g = jpeg_geom(H, W, hs, vs, components);
    f.hs = hs; f.vs = vs;
    f.nl = hs * vs;
    f.nz = f.nl + (components == 3 ? 2 : 0);
    f.mcus = f.g.mcus_x * f.g.mcus_y;
    return f;
}
// block z of MCU `mcu` (scan order) -> its index in the image's coefficient storage: the inverse of jpeg_block on the
// geometry of jpeg_geom, which both share
__host__ __device__ __forceinline__ int unpack_block_index(const unpack_frame& f, const int mcu, const int z) {
    const int my = mcu / f.g.mcus_x, mx = mcu - my * f.g.mcus_x;
    if (z < f.nl) {
        const int v = z / f.hs, u = z - v * f.hs;
        return (my * f.vs + v) * f.g.bw0 + mx * f.hs + u;
    }
    return f.g.n0 + (z - f.nl) * f.g.n1 + my * f.g.mcus_x + mx;
}

__host__ __device__ __forceinline__ unsigned unpack_nsub(const unsigned len, const int subseq_bits) {
    const unsigned n = (unsigned)(((unsigned long long)len * 8 + (unsigned)subseq_bits - 1) / (unsigned)subseq_bits);
    return n ? n : 1u;                                                             // an empty segment still has a thread that reports it
}

__host__ __device__ __forceinline__ bool unpack_stuffing(const unpack_seg& s, const unsigned i) {
    return i > 0 && i < s.len && s.data[i] == 0 && s.data[i - 1] == 0xFF;
}

// the position n >= 1 bits after p, stepping over stuffing; the caller has checked that the bits exist
__host__ __device__ __forceinline__ unsigned unpack_advance(const unpack_seg& s, const unsigned p, const int n) {
    const unsigned total = (p & 7) + (unsigned)n;
    unsigned i = p >> 3;
    for (unsigned c = total >> 3; c > 0; --c) {
        ++i;
        if (unpack_stuffing(s, i)) ++i;
    }
    return i * 8 + (total & 7);
}

// the guess a subsequence starts from: a DC code of MCU block 0 at its first bit (a subsequence that starts on stuffing
// skips it)
__host__ __device__ __forceinline__ unpack_state unpack_guess(const unpack_seg& s, const unsigned j, const int subseq_bits) {
    unpack_state st = {j * (unsigned)subseq_bits, 0, 0};
    if (unpack_stuffing(s, st.p >> 3)) st.p += 8;
    return st;
}

// the next 40 - (p & 7) >= 33 bits at p, left-aligned in 64, zero-padded past the end of the segment; avail: how many of
// them are data.  One step needs at most a 16-bit code and 15 extra bits.
__host__ __device__ __forceinline__ unsigned long long unpack_window(const unpack_seg& s, const unsigned p, int& avail) {
    unsigned i = p >> 3;
    unsigned long long w = 0;
    int got = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        w <<= 8;
        if (i < s.len) {
            w |= s.data[i];
            got += 8;
            ++i;
            if (unpack_stuffing(s, i)) ++i;
        }
    }
    avail = got - (int)(p & 7);
    return w << (24 + (p & 7));
}

// huff_decode of ssd_jpeg.hip on 16 peeked bits: the symbol and its code length, or -1: the code is not in the table.
// The masks only matter for tables no DHT segment gives (device memory the host cannot check): every index stays inside.
__host__ __device__ __forceinline__ int unpack_symbol(const huff_view& t, const unsigned v16, int& len) {
    const unsigned e = t.look[v16 >> 8];
    if (e) {
        len = (int)(e >> 8);
        return len <= 8 ? (int)(e & 255) : -1;
    }
    for (len = 9; len <= 16; ++len) {
        const int code = (int)(v16 >> (16 - len));
        if (code <= t.maxcode[len]) return t.vals[(unsigned)(t.valoff[len] + code) & 255u];
    }
    return -1;
}

__host__ __device__ __forceinline__ int unpack_extend(const int v, const int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

enum : int { kStepOk = 0, kStepBlockDone = 1, kStepError = 2, kStepEnd = 3 };

// ONE step: a DC or an AC symbol plus its extra bits at `st`, decode_block of ssd_jpeg.hip in every detail (ZRL, EOB,
// extend, k <= 63, no padding consumed).  It always moves p forward or ends the segment, so every loop over it is bounded
// by the bits of the segment:
//   kStepOk / kStepBlockDone  a symbol was taken (sink.value(k, v) for a nonzero value at zigzag index k; 0: the DC difference)
//   kStepError                a code outside its table or an index past 63 -- what the host decoder refuses.  A speculative
//                             start meets these all the time; the fixed rule is "skip one bit, keep z and k" (any rule
//                             does: exactness comes from the fixed point alone)
//   kStepEnd                  the bits ran out: p moves to the end of the segment
template <class Sink>
__host__ __device__ __forceinline__ int unpack_step(const unpack_seg& s, const huff_view& dc, const huff_view& ac, const int nz,
                                                    unpack_state& st, Sink& sink) {
    int avail, len;
    const unsigned long long w = unpack_window(s, st.p, avail);
    const int sym = unpack_symbol(st.k == 0 ? dc : ac, (unsigned)(w >> 48), len);
    if (sym < 0) { st.p = unpack_advance(s, st.p, 1); return kStepError; }
    if (len > avail) { st.p = s.len * 8; return kStepEnd; }
    int k = st.k, bits = sym & 15;
    bool done = false;
    if (k != 0) {
        const int r = sym >> 4;
        if (bits == 0) {
            if (r != 15) done = true;                                              // end of block
            else { k += 16; done = k > 63; }                                       // ZRL; past 63 the host's loop simply ends
        } else {
            k += r;
            if (k > 63) { st.p = unpack_advance(s, st.p, 1); return kStepError; }
        }
    }
    if (bits) {
        if (len + bits > avail) { st.p = s.len * 8; return kStepEnd; }
        const int v = (int)((w << len) >> (64 - bits));
        sink.value(k, unpack_extend(v, bits));
    }
    if (bits || k == 0) { ++k; done = done || k > 63; }
    st.p = unpack_advance(s, st.p, len + bits);
    if (done) { st.z = st.z + 1 == nz ? 0 : st.z + 1; st.k = 0; return kStepBlockDone; }
    st.k = k;
    return kStepOk;
}

struct unpack_no_sink {
    __host__ __device__ __forceinline__ void value(const int, const int) {}
};
struct unpack_store_sink {
    short* blk;                 // the block being decoded, nullptr: outside the image
    const unsigned char* zz;    // kZigzag
    __host__ __device__ __forceinline__ void value(const int k, const int v) { if (blk) blk[zz[k]] = (short)v; }
};

// component tables of MCU block z: tabs[2 c] DC, tabs[2 c + 1] AC
__host__ __device__ __forceinline__ int unpack_comp(const unpack_frame& f, const int z) { return z < f.nl ? 0 : z - f.nl + 1; }

// Phase a, one thread, one sweep: from the entry state to the first state at or past end_bit, counting the blocks it
// completes on the way.
__host__ __device__ __forceinline__ unpack_state unpack_sweep(const unpack_seg& s, const ssd_jpeg_huff* tabs, const unpack_frame& f,
                                                              unpack_state st, const unsigned end_bit, unsigned& completed) {
    unpack_no_sink sink;
    completed = 0;
    while (st.p < end_bit) {
        const int c = unpack_comp(f, st.z);
        if (unpack_step(s, huff_view_of(tabs + 2 * c), huff_view_of(tabs + 2 * c + 1), f.nz, st, sink) == kStepBlockDone) ++completed;
    }
    return st;
}

// Phase c, one thread: decode once more from the settled entry state, whose block is number `ordinal` of the segment, and
// store the AC values and the DC DIFFERENCES of the blocks below seg_blocks (every store inside the image's storage: the
// MCU is checked against the frame).  Returns the kUnpack* flags of what the host decoder refuses.
__host__ __device__ __forceinline__ int unpack_write(const unpack_seg& s, const ssd_jpeg_huff* tabs, const unpack_frame& f,
                                                     const unsigned char* zz, unpack_state st, const unsigned end_bit, unsigned ordinal,
                                                     const unsigned seg_blocks, const int first_mcu, const bool last_sub,
                                                     const bool last_seg, short* coef) {
    if (st.z < 0 || st.z >= f.nz || st.k < 0 || st.k > 63 || (int)(ordinal % (unsigned)f.nz) != st.z) return kUnpackTables;
    int flags = 0;
    long mcu = (long)first_mcu + ordinal / (unsigned)f.nz;
    unpack_store_sink sink = {nullptr, zz};
    while (st.p < end_bit && ordinal < seg_blocks) {
        sink.blk = mcu >= 0 && mcu < f.mcus ? coef + (long)unpack_block_index(f, (int)mcu, st.z) * 64 : nullptr;
        const int c = unpack_comp(f, st.z);
        const int r = unpack_step(s, huff_view_of(tabs + 2 * c), huff_view_of(tabs + 2 * c + 1), f.nz, st, sink);
        if (r == kStepError) flags |= kUnpackBadCode;
        else if (r == kStepEnd) flags |= kUnpackShort;
        else if (r == kStepBlockDone) {
            ++ordinal;
            if (st.z == 0) ++mcu;
            if (ordinal == seg_blocks && !last_seg) {
                // the host decoder finds RSTn where it looks only if it has fetched the segment's last byte: at least as
                // strict is "the interval's last code ends inside that byte"
                unsigned e = (st.p + 7) >> 3;
                if (unpack_stuffing(s, e)) ++e;
                if (e != s.len) flags |= kUnpackEarly;
            }
        }
    }
    if (last_sub && ordinal < seg_blocks) flags |= kUnpackShort;
    return flags;
}

// Phase d: where element e of component c's scan order (MCU order, NOT plane raster order) keeps its DC term, as an int16
// index into the image's storage; per: the component's blocks per MCU.
__host__ __device__ __forceinline__ long unpack_dc_at(const unpack_frame& f, const int c, const int per, const int e) {
    const int mcu = e / per, r = e - mcu * per;
    return (long)unpack_block_index(f, mcu, c == 0 ? r : f.nl + c - 1) * 64;
}

}  // namespace ssd
