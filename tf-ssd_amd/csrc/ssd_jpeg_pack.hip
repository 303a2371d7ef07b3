// The third stage of JPEG encoding on the device ("JPEG encoding: what runs where"): the quantised
// coefficients ssd_jpeg_forward wrote -> the complete streams of the batch, back to back, ssd_jpeg_entropy_encode's bytes
// bit for bit.  Huffman ENCODING is not serial: a block's code string depends on its own 64 coefficients and one
// neighbouring DC value, where it lands is a prefix sum of bit lengths, and byte stuffing is a second prefix sum over the
// 0xFF bytes.  Six kernels and two fills per call, whatever the batch (include/ssd_hip.h spells the contract out):
//   1 length   one thread per EMITTED block (one index space over the batch): bit length, 256-block sums
//   2 scan     one workgroup: exclusive scan of the sums (64-bit), every image's first bit
//   3 write    re-derives the codes, ORs them as big-endian words into the image's zeroed unstuffed stream (atomic OR:
//              neighbouring blocks share words, and OR commutes, so the bytes do not depend on scheduling)
//   4 count    one thread per 224-byte slot of the unstuffed streams (the same index space): its 0xFF bytes, 256-slot sums
//   5 scan     one workgroup: scan of those sums, every stream's size, the scan of the sizes = offsets_dev
//   6 scatter  every slot's bytes to their stuffed, final position; the header in front, EOI behind
// No workgroup waits on another; every scan is reduce, then scan, in separate launches on the one stream.
#include <climits>
#include <cstring>

#include "ssd_jpeg_common.h"

namespace ssd {

static const int kPackChunk = 256;          // blocks / slots per workgroup of kernels 1, 3, 4, 6
static const int kPackSlot = 224;           // bytes of unstuffed stream per block at the worst: 1660 bits + the padding, a multiple of 16
static const int kPackScanThreads = 1024;   // the one workgroup of kernels 2 and 5
static const int kPackBlockWords = 33;      // a staged block in LDS: 32 words + 1, so that the threads' rows fall into different banks

// code | length << 16 per symbol, built on the host from kStdHuff and handed to the kernels by value (2208 bytes of kernel
// arguments): no device-side global, no upload
struct pack_tables {
    unsigned dc[2][12];
    unsigned ac[2][256];
    unsigned zz[16];            // kZigzag, four entries a word
};

static pack_tables pack_build_tables() {
    pack_tables t;
    memset(&t, 0, sizeof(t));
    for (int i = 0; i < 64; ++i) t.zz[i >> 2] |= (unsigned)kZigzag[i] << (8 * (i & 3));
    for (int i = 0; i < 4; ++i) {
        const std_huff& s = kStdHuff[i];
        const int id = s.cls_id & 1;
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int j = 0; j < s.bits[len - 1]; ++j, ++k, ++code) {
                const unsigned e = code | ((unsigned)len << 16);
                if (s.cls_id >> 4) t.ac[id][s.vals[k]] = e; else t.dc[id][s.vals[k]] = e;
            }
            code <<= 1;
        }
    }
    return t;
}

// where the parts of the workspace begin (bytes, each a multiple of 16); the same on the host and in the kernels' arguments
struct pack_workspace {
    size_t len, part, part_excl, bit_base, ff, ff_part, ff_part_excl, ff_base, raw, total;
};
static pack_workspace pack_layout(const long blocks, const int B) {
    const size_t n = (size_t)blocks, p = (size_t)((blocks + kPackChunk - 1) / kPackChunk) + 1, b = (size_t)B + 1;
    pack_workspace w;
    size_t at = 0;
    auto part = [&](const size_t bytes) { const size_t here = at; at = align_up(at + bytes, 16); return here; };
    w.len = part(n * 4); w.part = part(p * 8); w.part_excl = part(p * 8); w.bit_base = part(b * 8);
    w.ff = part(n * 4); w.ff_part = part(p * 4); w.ff_part_excl = part(p * 4); w.ff_base = part(b * 4);
    w.raw = part(n * kPackSlot);
    w.total = at;
    return w;
}

__host__ __device__ __forceinline__ jpeg_geometry jpeg_geom(const ssd_jpeg_pack_desc& d) {
    return jpeg_geom(d.H, d.W, d.h_samp, d.v_samp, 3);
}

// Block r of MCU `mcu` in emission order (the luma blocks row by row, then Cb, then Cr): its component, where its 64
// coefficients begin in the image's storage (int16 index; always inside the storage), and whether it is a REAL block.
__device__ __forceinline__ bool pack_locate(const ssd_jpeg_pack_desc& d, const jpeg_geometry& g, const int mcu, const int r, int& comp,
                                            long& at) {
    const int nl = d.h_samp * d.v_samp;
    const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
    int by, bx, bw, rw, rh;
    long plane;
    if (r < nl) {
        comp = 0;
        const int v = r / d.h_samp, u = r - v * d.h_samp;
        by = my * d.v_samp + v; bx = mx * d.h_samp + u; bw = g.bw0;
        rw = (d.W + 7) / 8; rh = (d.H + 7) / 8;
        plane = 0;
    } else {
        comp = 1 + r - nl;
        by = my; bx = mx; bw = g.mcus_x;
        rw = ((d.W + d.h_samp - 1) / d.h_samp + 7) / 8; rh = ((d.H + d.v_samp - 1) / d.v_samp + 7) / 8;
        plane = (long)g.n0 + (long)(comp - 1) * g.n1;
    }
    at = (plane + (long)by * bw + bx) * 64;
    return by < rh && bx < rw;
}

__device__ __forceinline__ int pack_category(const int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __clz(a) : 0;
}

struct pack_count_sink {
    unsigned bits;
    __device__ __forceinline__ void put(const unsigned, const int len) { bits += (unsigned)len; }
};

// Bits, most significant first, into big-endian 32-bit words of a zeroed stream that other threads write too: every word
// leaves as one atomic OR.  `cur` holds the `fill` bits not yet written at its top.
struct pack_word_sink {
    unsigned* words;
    long at;
    unsigned cur;
    int fill;
    __device__ __forceinline__ void flush() { atomicOr(words + at, __builtin_bswap32(cur)); ++at; }
    // value < 2^len, 1 <= len <= 31
    __device__ __forceinline__ void put(const unsigned value, const int len) {
        const int room = 32 - fill;
        if (len < room) {
            cur |= value << (room - len);
            fill += len;
        } else {
            cur |= value >> (len - room);
            flush();
            fill = len - room;
            cur = fill ? value << (32 - fill) : 0u;
        }
    }
    __device__ __forceinline__ void finish() { if (fill) flush(); }
};

// One block's code string into `s`: the DC difference, then run-length / category coding of the AC terms in zigzag order.
// What ssd_jpeg_entropy_encode refuses -- a DC difference beyond category 11 (bit 0 of the answer), an AC term beyond
// category 10 (bit 1) -- is coded as zero, so that a block never exceeds 1660 bits and kernels 1 and 3 agree.
template <class Sink>
__device__ __forceinline__ int pack_code_block(Sink& s, const unsigned* __restrict__ dct, const unsigned* __restrict__ act,
                                               const short* __restrict__ blk, const unsigned char* __restrict__ zz, const bool dummy,
                                               int diff) {
    int flags = 0;
    int n = pack_category(diff);
    if (n > 11) { flags |= 1; diff = 0; n = 0; }
    unsigned e = dct[n];
    s.put(((e & 0xFFFFu) << n) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1)), (int)(e >> 16) + n);
    const unsigned eob = act[0];
    if (dummy) {
        s.put(eob & 0xFFFFu, (int)(eob >> 16));
        return flags;
    }
    const unsigned zrl = act[0xF0];
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        int v = blk[zz[k]];
        n = pack_category(v);
        if (n > 10) { flags |= 2; v = 0; }
        if (v == 0) { ++run; continue; }
        for (; run > 15; run -= 16) s.put(zrl & 0xFFFFu, (int)(zrl >> 16));
        e = act[(run << 4) | n];
        s.put(((e & 0xFFFFu) << n) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1)), (int)(e >> 16) + n);
        run = 0;
    }
    if (run) s.put(eob & 0xFFFFu, (int)(eob >> 16));
    return flags;
}

struct pack_lds {
    unsigned dc[2][12];
    unsigned ac[2][256];
    unsigned char zz[64];
    unsigned wave[4];
    unsigned blk[kPackChunk][kPackBlockWords];
};

// what kernels 1 and 3 know about their thread's block
struct pack_block {
    int b, local, nblocks, comp, diff;
    long long block_start;
    bool live, dummy;
};

// The prologue kernels 1 and 3 share: the tables into LDS; the thread's emitted block -> image, MCU, component; a real
// block's coefficients staged in the thread's LDS row (eight aligned 16-byte loads) and its DC difference against the DC of
// the block emitted before it in the same component -- a dummy block repeats that DC, so the walk back skips dummies and
// ends on a real block's value; a dummy block itself has a difference of zero and reads nothing.
__device__ __forceinline__ pack_block pack_prepare(pack_lds& L, const pack_tables& T, const short* __restrict__ coef,
                                                   const ssd_jpeg_pack_desc* __restrict__ desc, const int B, const int total) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 24; i += kPackChunk) (&L.dc[0][0])[i] = (&T.dc[0][0])[i];
    for (int i = tid; i < 512; i += kPackChunk) (&L.ac[0][0])[i] = (&T.ac[0][0])[i];
    if (tid < 64) L.zz[tid] = (unsigned char)(T.zz[tid >> 2] >> (8 * (tid & 3)));
    pack_block k;
    const int blk = blockIdx.x * kPackChunk + tid;
    k.live = blk < total;
    k.b = 0; k.local = 0; k.nblocks = 0; k.comp = 0; k.diff = 0; k.block_start = 0; k.dummy = true;
    if (k.live) {
        k.b = find_image(B, blk, [&](const int i) { return desc[i].block_start; });
        const ssd_jpeg_pack_desc d = desc[k.b];
        const jpeg_geometry g = jpeg_geom(d);
        k.block_start = d.block_start;
        k.local = blk - d.block_start;
        k.nblocks = g.nblocks;
        const int per = d.h_samp * d.v_samp + 2;
        const int mcu = k.local / per, r = k.local - mcu * per;
        long at;
        k.dummy = !pack_locate(d, g, mcu, r, k.comp, at);
        if (!k.dummy) {
            const short* image = coef + d.coef_offset / 2;
            const uint4* src = reinterpret_cast<const uint4*>(image + at);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint4 w = src[i];
                L.blk[tid][4 * i] = w.x; L.blk[tid][4 * i + 1] = w.y; L.blk[tid][4 * i + 2] = w.z; L.blk[tid][4 * i + 3] = w.w;
            }
            int pm = mcu, pr = r;
            if (k.comp == 0 && r > 0) pr = r - 1;
            else { pm = mcu - 1; if (k.comp == 0) pr = d.h_samp * d.v_samp - 1; }
            int pred = 0;
            if (pm >= 0) {
                int c2;
                long at2;
                bool real = pack_locate(d, g, pm, pr, c2, at2);
                while (!real && c2 == 0 && pr > 0) { --pr; real = pack_locate(d, g, pm, pr, c2, at2); }
                pred = image[at2];
            }
            k.diff = (int)(short)(L.blk[tid][0] & 0xFFFFu) - pred;
        }
    }
    return k;
}

// exclusive prefix of v over the 256 threads of the workgroup and their total; every thread calls it
__device__ __forceinline__ unsigned pack_chunk_scan(const unsigned v, unsigned* wave_sums, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    unsigned base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kPackChunk / 64; ++w) {
        const unsigned s = wave_sums[w];
        if (w < wave) base += s;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

// Kernel 1: every emitted block's bit length, the sum of each 256, and the status bits of what the baseline cannot code.
__global__ __launch_bounds__(256) void jpeg_pack_length_kernel(const short* __restrict__ coef, const ssd_jpeg_pack_desc* __restrict__ desc,
                                                              const int B, const int total, const pack_tables T,
                                                              unsigned* __restrict__ len, unsigned long long* __restrict__ part,
                                                              int* __restrict__ status) {
    __shared__ pack_lds L;
    const pack_block k = pack_prepare(L, T, coef, desc, B, total);
    __syncthreads();
    pack_count_sink s = {0};
    if (k.live) {
        const int t = k.comp ? 1 : 0;
        const int flags = pack_code_block(s, L.dc[t], L.ac[t], reinterpret_cast<const short*>(L.blk[threadIdx.x]), L.zz, k.dummy, k.diff);
        len[blockIdx.x * kPackChunk + threadIdx.x] = s.bits;
        if (flags) atomicOr(status + k.b, flags);
    }
    unsigned sum;
    pack_chunk_scan(s.bits, L.wave, sum);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// inclusive -> exclusive scan over the kPackScanThreads threads of the one workgroup, through LDS
template <typename T>
__device__ __forceinline__ T pack_wide_scan(const T v, T* s, T& total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < kPackScanThreads; o <<= 1) {
        const T t = tid >= o ? s[tid - o] : (T)0;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    const T inc = s[tid];
    total = s[kPackScanThreads - 1];
    __syncthreads();
    return inc - v;
}

// The scan both one-workgroup kernels begin with: part[0..P) -> its exclusive prefix in excl[0..P], excl[P] the total; then
// base[b] for b <= B: the prefix at image b's first element (block_start; the batch's total for b == B), from the prefix of
// its 256-chunk and the elements of that chunk before it.
template <typename T>
__device__ __forceinline__ void pack_scan_parts(const T* __restrict__ part, T* __restrict__ excl, const int P, const unsigned* __restrict__ elem,
                                                const ssd_jpeg_pack_desc* __restrict__ desc, const int B, const int total,
                                                T* __restrict__ base, T* s) {
    const int tid = threadIdx.x;
    const int per = (P + kPackScanThreads - 1) / kPackScanThreads;
    const int lo = min(tid * per, P), hi = min(lo + per, P);
    T sum = 0;
    for (int i = lo; i < hi; ++i) sum += part[i];
    T all;
    T run = pack_wide_scan(sum, s, all);
    for (int i = lo; i < hi; ++i) { excl[i] = run; run += part[i]; }
    if (tid == 0) excl[P] = all;
    __syncthreads();                                                              // excl is read below by other threads of this workgroup
    for (int b = tid; b <= B; b += kPackScanThreads) {
        const int first = b < B ? desc[b].block_start : total;
        const int c = first / kPackChunk;
        T v = excl[c];
        for (int i = c * kPackChunk; i < first; ++i) v += elem[i];
        base[b] = v;
    }
}

// Kernel 2: one workgroup.  Bit offsets are 64-bit: a batch within the 2^31 - 1 byte bound can hold more than 2^32 bits.
__global__ __launch_bounds__(1024) void jpeg_pack_scan_bits_kernel(const unsigned long long* __restrict__ part,
                                                                  unsigned long long* __restrict__ part_excl, const int P,
                                                                  const unsigned* __restrict__ len, const ssd_jpeg_pack_desc* __restrict__ desc,
                                                                  const int B, const int total, unsigned long long* __restrict__ bit_base) {
    __shared__ unsigned long long s[kPackScanThreads];
    pack_scan_parts(part, part_excl, P, len, desc, B, total, bit_base, s);
}

// Kernel 3: the codes again, ORed into the image's unstuffed stream at the block's bit offset; the image's last block pads
// the last byte with 1-bits.
__global__ __launch_bounds__(256) void jpeg_pack_write_kernel(const short* __restrict__ coef, const ssd_jpeg_pack_desc* __restrict__ desc,
                                                             const int B, const int total, const pack_tables T,
                                                             const unsigned* __restrict__ len, const unsigned long long* __restrict__ part_excl,
                                                             const unsigned long long* __restrict__ bit_base, unsigned char* __restrict__ raw) {
    __shared__ pack_lds L;
    const pack_block k = pack_prepare(L, T, coef, desc, B, total);
    const unsigned bits = k.live ? len[blockIdx.x * kPackChunk + threadIdx.x] : 0u;
    unsigned sum;
    const unsigned before = pack_chunk_scan(bits, L.wave, sum);                   // its barriers also order the tables' staging
    if (!k.live) return;
    const unsigned long long at = part_excl[blockIdx.x] + before - bit_base[k.b];   // bits from the image's first
    pack_word_sink s = {reinterpret_cast<unsigned*>(raw + k.block_start * kPackSlot), (long)(at >> 5), 0u, (int)(at & 31)};
    const int t = k.comp ? 1 : 0;
    pack_code_block(s, L.dc[t], L.ac[t], reinterpret_cast<const short*>(L.blk[threadIdx.x]), L.zz, k.dummy, k.diff);
    if (k.local == k.nblocks - 1) {
        const int pad = (int)((0ull - (at + bits)) & 7);
        if (pad) s.put((1u << pad) - 1, pad);
    }
    s.finish();
}

// what kernels 4 and 6 know about their thread's slot: the image, and which bytes of its unstuffed stream the slot holds
struct pack_slot {
    int b, local, nblocks, n;         // n: bytes of the stream in this slot, 0..kPackSlot
    long long block_start, stream_bytes;
    bool live;
};
__device__ __forceinline__ pack_slot pack_find_slot(const ssd_jpeg_pack_desc* __restrict__ desc, const int B, const int total,
                                                    const unsigned long long* __restrict__ bit_base) {
    pack_slot k;
    const int slot = blockIdx.x * kPackChunk + threadIdx.x;
    k.live = slot < total;
    k.b = 0; k.local = 0; k.nblocks = 0; k.n = 0; k.block_start = 0; k.stream_bytes = 0;
    if (k.live) {
        k.b = find_image(B, slot, [&](const int i) { return desc[i].block_start; });
        const ssd_jpeg_pack_desc d = desc[k.b];
        k.block_start = d.block_start;
        k.local = slot - d.block_start;
        k.nblocks = jpeg_geom(d).nblocks;
        k.stream_bytes = (long long)((bit_base[k.b + 1] - bit_base[k.b] + 7) >> 3);
        const long long left = k.stream_bytes - (long long)k.local * kPackSlot;
        k.n = (int)(left < 0 ? 0 : (left > kPackSlot ? kPackSlot : left));
    }
    return k;
}

__device__ __forceinline__ unsigned pack_count_ff(const unsigned w) {
    return (unsigned)((w & 0xFFu) == 0xFFu) + (unsigned)((w & 0xFF00u) == 0xFF00u) + (unsigned)((w & 0xFF0000u) == 0xFF0000u) +
           (unsigned)((w >> 24) == 0xFFu);
}

// Kernel 4: the 0xFF bytes of every slot (the stream's bytes past its end are zero, so whole 16-byte pieces are counted).
__global__ __launch_bounds__(256) void jpeg_pack_count_kernel(const ssd_jpeg_pack_desc* __restrict__ desc, const int B, const int total,
                                                             const unsigned long long* __restrict__ bit_base,
                                                             const unsigned char* __restrict__ raw, unsigned* __restrict__ ff,
                                                             unsigned* __restrict__ ff_part) {
    __shared__ unsigned wave[4];
    const pack_slot k = pack_find_slot(desc, B, total, bit_base);
    unsigned count = 0;
    if (k.live) {
        const uint4* src = reinterpret_cast<const uint4*>(raw + (k.block_start + k.local) * kPackSlot);
        for (int i = 0; i * 16 < k.n; ++i) {
            const uint4 w = src[i];
            count += pack_count_ff(w.x) + pack_count_ff(w.y) + pack_count_ff(w.z) + pack_count_ff(w.w);
        }
        ff[blockIdx.x * kPackChunk + threadIdx.x] = count;
    }
    unsigned sum;
    pack_chunk_scan(count, wave, sum);
    if (threadIdx.x == 0) ff_part[blockIdx.x] = sum;
}

// Kernel 5: one workgroup.  The scan of the 0xFF counts, then every stream's size -- header + data + stuffing + EOI -- and
// the scan of the sizes over the batch: offsets[0..B].
__global__ __launch_bounds__(1024) void jpeg_pack_scan_sizes_kernel(const unsigned* __restrict__ ff_part, unsigned* __restrict__ ff_part_excl,
                                                                   const int P, const unsigned* __restrict__ ff,
                                                                   const ssd_jpeg_pack_desc* __restrict__ desc, const int B, const int total,
                                                                   unsigned* __restrict__ ff_base,
                                                                   const unsigned long long* __restrict__ bit_base, int* __restrict__ offsets) {
    __shared__ unsigned s[kPackScanThreads];
    pack_scan_parts(ff_part, ff_part_excl, P, ff, desc, B, total, ff_base, s);
    __syncthreads();                                                              // ff_base is read below by other threads of this workgroup
    const int tid = threadIdx.x;
    const int per = (B + kPackScanThreads - 1) / kPackScanThreads;
    const int lo = min(tid * per, B), hi = min(lo + per, B);
    auto size_of = [&](const int b) {
        return (unsigned)kEncHeaderBytes + (unsigned)((bit_base[b + 1] - bit_base[b] + 7) >> 3) + (ff_base[b + 1] - ff_base[b]) + 2u;
    };
    unsigned sum = 0;
    for (int b = lo; b < hi; ++b) sum += size_of(b);
    unsigned all;
    unsigned run = pack_wide_scan(sum, s, all);
    for (int b = lo; b < hi; ++b) { offsets[b] = (int)run; run += size_of(b); }
    if (tid == 0) offsets[B] = (int)all;
}

// Kernel 6: every slot's bytes to offsets[b] + header + (bytes before the slot) + (0xFF bytes before the slot), a zero
// after every 0xFF; the slot that holds the stream's last byte adds EOI; the image's slots share the copy of its header.
__global__ __launch_bounds__(256) void jpeg_pack_scatter_kernel(const ssd_jpeg_pack_desc* __restrict__ desc, const int B, const int total,
                                                               const unsigned long long* __restrict__ bit_base,
                                                               const unsigned char* __restrict__ raw, const unsigned* __restrict__ ff,
                                                               const unsigned* __restrict__ ff_part_excl, const unsigned* __restrict__ ff_base,
                                                               const int* __restrict__ offsets, const unsigned char* __restrict__ packed,
                                                               unsigned char* __restrict__ out) {
    __shared__ unsigned wave[4];
    const pack_slot k = pack_find_slot(desc, B, total, bit_base);
    const unsigned count = k.live ? ff[blockIdx.x * kPackChunk + threadIdx.x] : 0u;
    unsigned sum;
    const unsigned before = pack_chunk_scan(count, wave, sum);
    if (!k.live) return;
    unsigned char* stream = out + offsets[k.b];
    if (k.n > 0) {
        const unsigned stuffed = ff_part_excl[blockIdx.x] + before - ff_base[k.b];  // 0xFF bytes of the image before this slot
        unsigned char* dst = stream + kEncHeaderBytes + (long)k.local * kPackSlot + stuffed;
        const uint4* src = reinterpret_cast<const uint4*>(raw + (k.block_start + k.local) * kPackSlot);
        for (int i = 0; i * 16 < k.n; ++i) {
            const uint4 w4 = src[i];
            const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (i * 16 + j < k.n) {
                    const unsigned byte = (w[j >> 2] >> (8 * (j & 3))) & 255u;
                    *dst++ = (unsigned char)byte;
                    if (byte == 0xFFu) *dst++ = 0;
                }
            }
        }
        if ((long long)k.local * kPackSlot + k.n == k.stream_bytes) { dst[0] = 0xFF; dst[1] = 0xD9; }
    }
    const unsigned char* header = packed + desc[k.b].header_offset;
    for (int i = k.local; i < (int)kEncHeaderBytes; i += k.nblocks) stream[i] = header[i];
}

static const char* const kPackName = "ssd_jpeg_pack";

}  // namespace ssd

using namespace ssd;

// the batch's emitted blocks, or -1 for a batch no call would take
static long pack_total_blocks(const ssd_jpeg_pack_desc* desc_host, const int B) {
    long blocks = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_pack_desc& d = desc_host[b];
        if (!image_side_ok(d.H) || !image_side_ok(d.W) || !jpeg_sampling_ok(d.h_samp, d.v_samp)) return -1;
        blocks += jpeg_geom(d).nblocks;
    }
    return blocks;
}

extern "C" size_t ssd_jpeg_pack_workspace_bytes(const struct ssd_jpeg_pack_desc* desc_host, int B) {
    if (!desc_host || B <= 0 || B > 65535) return 0;
    const long blocks = pack_total_blocks(desc_host, B);
    return blocks < 0 ? 0 : pack_layout(blocks, B).total;
}

extern "C" int ssd_jpeg_pack(const short* coef_dev, size_t coef_bytes, const unsigned char* packed_dev, size_t packed_bytes,
                             const struct ssd_jpeg_pack_desc* desc_host, const struct ssd_jpeg_pack_desc* desc_dev, int B,
                             unsigned char* out_dev, size_t out_bytes, int* offsets_dev, int* status_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0, "%s: bad batch", kPackName);
    SSD_UNSUPPORTED_IF(B > 65535, "%s: B = %d (at most 65535)", kPackName, B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(coef_dev && packed_dev && desc_host && desc_dev && out_dev && offsets_dev && status_dev && workspace_dev,
                  "%s: NULL pointer", kPackName);
    SSD_CHECK_ARG((((size_t)coef_dev | (size_t)packed_dev | (size_t)out_dev | (size_t)workspace_dev) & 15) == 0,
                  "%s: a buffer is not 16-byte aligned", kPackName);
    SSD_CHECK_ARG((((size_t)offsets_dev | (size_t)status_dev) & 3) == 0, "%s: offsets_dev / status_dev are not 4-byte aligned", kPackName);
    long blocks = 0;
    size_t coef_end = 0, bound = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_pack_desc& d = desc_host[b];
        SSD_UNSUPPORTED_IF(!image_side_ok(d.H) || !image_side_ok(d.W), "%s: image %d is %d x %d, outside 1..%d", kPackName, b, d.H, d.W,
                           kMaxImageSide);
        SSD_UNSUPPORTED_IF(!jpeg_sampling_ok(d.h_samp, d.v_samp), "%s: image %d: luma sampling %dx%d (1x1, 2x1 and 2x2 only)", kPackName, b,
                           d.h_samp, d.v_samp);
        const size_t nb = (size_t)jpeg_geom(d).nblocks;
        SSD_CHECK_ARG(region_ok(d.coef_offset, nb * 128, coef_bytes, 16, &coef_end),
                      "%s: image %d: coefficients outside coef_dev, misaligned or overlapping", kPackName, b);
        SSD_CHECK_ARG(region_ok(d.header_offset, kEncHeaderBytes, packed_bytes, 16), "%s: image %d: header outside packed_dev or misaligned",
                      kPackName, b);
        SSD_CHECK_ARG(d.block_start == blocks, "%s: image %d: block_start is not the running sum", kPackName, b);
        blocks += (long)nb;
        bound += align_up(jpeg_encode_bound_bytes(nb), 16);
        SSD_UNSUPPORTED_IF(bound > (size_t)INT_MAX, "%s: the streams may need more than 2^31 - 1 bytes (image %d)", kPackName, b);
    }
    SSD_CHECK_ARG(out_bytes >= bound, "%s: out holds %zu bytes, the batch may need %zu", kPackName, out_bytes, bound);
    const pack_workspace w = pack_layout(blocks, B);
    SSD_CHECK_ARG(workspace_bytes >= w.total, "%s: the workspace holds %zu bytes, the batch needs %zu", kPackName, workspace_bytes, w.total);
    static const pack_tables tables = pack_build_tables();
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace_dev;
    unsigned* len = (unsigned*)(ws + w.len);
    unsigned long long* part = (unsigned long long*)(ws + w.part);
    unsigned long long* part_excl = (unsigned long long*)(ws + w.part_excl);
    unsigned long long* bit_base = (unsigned long long*)(ws + w.bit_base);
    unsigned* ff = (unsigned*)(ws + w.ff);
    unsigned* ff_part = (unsigned*)(ws + w.ff_part);
    unsigned* ff_part_excl = (unsigned*)(ws + w.ff_part_excl);
    unsigned* ff_base = (unsigned*)(ws + w.ff_base);
    unsigned char* raw = ws + w.raw;
    const int total = (int)blocks, P = (total + kPackChunk - 1) / kPackChunk;
    const dim3 grid((unsigned)P), chunk(kPackChunk), one(1), wide(kPackScanThreads);
    SSD_HIP(hipMemsetAsync(ws, 0, w.total, st));
    SSD_HIP(hipMemsetAsync(status_dev, 0, (size_t)B * 4, st));
    hipLaunchKernelGGL(jpeg_pack_length_kernel, grid, chunk, 0, st, coef_dev, desc_dev, B, total, tables, len, part, status_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_scan_bits_kernel, one, wide, 0, st, (const unsigned long long*)part, part_excl, P, (const unsigned*)len,
                       desc_dev, B, total, bit_base);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_write_kernel, grid, chunk, 0, st, coef_dev, desc_dev, B, total, tables, (const unsigned*)len,
                       (const unsigned long long*)part_excl, (const unsigned long long*)bit_base, raw);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_count_kernel, grid, chunk, 0, st, desc_dev, B, total, (const unsigned long long*)bit_base,
                       (const unsigned char*)raw, ff, ff_part);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_scan_sizes_kernel, one, wide, 0, st, (const unsigned*)ff_part, ff_part_excl, P, (const unsigned*)ff, desc_dev,
                       B, total, ff_base, (const unsigned long long*)bit_base, offsets_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_scatter_kernel, grid, chunk, 0, st, desc_dev, B, total, (const unsigned long long*)bit_base,
                       (const unsigned char*)raw, (const unsigned*)ff, (const unsigned*)ff_part_excl, (const unsigned*)ff_base,
                       (const int*)offsets_dev, packed_dev, out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
