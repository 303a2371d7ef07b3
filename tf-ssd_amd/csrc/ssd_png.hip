// PNG encoding on the device ("PNG encoding"): uint8 RGB pixels of a ragged batch -> the finished
// files, back to back in one device buffer; and the host model that writes the same bytes from the same step functions
// (ssd_png_common.h).  The format is fixed in include/ssd_hip.h: per-row filters, the filtered stream cut into 16384-byte
// segments, one deflate block of distance-1 matches (or a stored block) and one IDAT chunk per segment.  Four kernels per
// call, whatever the batch:
//   1 filter   one workgroup per (image, row): the adaptive choice is five sums over the row; the row goes to the workspace
//   2 segment  one workgroup per segment (one index space over the batch): the phases of ssd_png_common.h with a barrier
//              between them -- runs, token histogram, the two codes, the choice between dynamic and stored, the bits ORed
//              into LDS, the chunk's CRC register and the Adler-32 sums -- and the finished data to the segment's slot
//   3 scan     one workgroup: the chunk sizes -> every chunk's place, every file's size and Adler-32, offsets_dev
//   4 scatter  one workgroup per segment: length, "IDAT", the slot's bytes, CRC to their final place; an image's first
//              segment adds the signature and IHDR, its last the Adler-32 and IEND
// No workgroup waits on another; what the threads of a workgroup share is summed or ORed with integer LDS atomics, so the
// bytes do not depend on scheduling.
#include <climits>
#include <cstring>
#include <vector>

#include "ssd_jpeg_common.h"
#include "ssd_png_common.h"

namespace ssd {

static const int kPngScanThreads = 1024;    // the one workgroup of kernel 3

__host__ __device__ __forceinline__ bool png_filter_ok(const int f) { return f >= 0 && f <= 5; }

// where the parts of the workspace begin (bytes, each a multiple of 16)
struct png_workspace {
    size_t filtered, slots, meta, excl, adler, total;
};
static png_workspace png_layout(const long segs, const int B) {
    png_workspace w;
    size_t at = 0;
    auto part = [&](const size_t bytes) { const size_t here = at; at = align_up(at + bytes, 16); return here; };
    w.filtered = part((size_t)segs * kPngSeg);
    w.slots = part((size_t)segs * kPngSlot);
    w.meta = part((size_t)segs * 16);
    w.excl = part(((size_t)segs + 1) * 4);
    w.adler = part((size_t)B * 4);
    w.total = at;
    return w;
}

// Kernel 1: row y of image b, filtered, to its place in the image's filtered stream (which begins at its first segment).
// A workgroup takes the rows blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(256) void png_filter_kernel(const unsigned char* __restrict__ rgb, const ssd_png_desc* __restrict__ desc, const int B,
                                                        const int rows, unsigned char* __restrict__ filtered) {
    __shared__ unsigned sums[5];
    const int tid = threadIdx.x;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int b = find_image(B, (int)row, [&](const int i) { return desc[i].row_start; });
        const ssd_png_desc d = desc[b];
        const int y = (int)row - d.row_start, n = 3 * d.W;
        const unsigned char* src = rgb + d.src_offset + (long long)y * n;
        const unsigned char* up = src - n;                                         // read for y > 0 only
        unsigned char* dst = filtered + (long long)d.seg_start * kPngSeg + (long long)y * (n + 1);
        int type = d.filter;
        if (type == 5) {
            if (tid < 5) sums[tid] = 0;
            __syncthreads();
            unsigned mine[5] = {0, 0, 0, 0, 0};
            for (int x = tid; x < n; x += 256) {
                const int v = src[x], a = x >= 3 ? src[x - 3] : 0, bb = y ? up[x] : 0, c = (y && x >= 3) ? up[x - 3] : 0;
#pragma unroll
                for (int t = 0; t < 5; ++t) mine[t] += png_cost(png_filter(t, v, a, bb, c));
            }
#pragma unroll
            for (int t = 0; t < 5; ++t) atomicAdd(&sums[t], mine[t]);
            __syncthreads();
            type = png_pick_filter(sums);
            __syncthreads();                                                      // the next row zeroes the sums
        }
        if (tid == 0) dst[0] = (unsigned char)type;
        for (int x = tid; x < n; x += 256) {
            const int v = src[x], a = x >= 3 ? src[x - 3] : 0, bb = y ? up[x] : 0, c = (y && x >= 3) ? up[x - 3] : 0;
            dst[1 + x] = (unsigned char)png_filter(type, v, a, bb, c);
        }
    }
}

// what kernels 2 and 4 know about their workgroup's segment
struct png_seg_place {
    int b, len, is_first, is_last;
};
__device__ __forceinline__ png_seg_place png_find_segment(const ssd_png_desc* __restrict__ desc, const int B, const int g) {
    png_seg_place p;
    p.b = find_image(B, g, [&](const int i) { return desc[i].seg_start; });
    const ssd_png_desc d = desc[p.b];
    const long long bytes = png_stream_bytes(d.H, d.W), at = (long long)(g - d.seg_start) * kPngSeg;
    p.len = (int)(bytes - at < kPngSeg ? bytes - at : kPngSeg);
    p.is_first = g == d.seg_start;
    p.is_last = at + p.len == bytes;
    return p;
}

// Kernel 2: segment g.  meta[g] = (bytes of chunk data, the CRC register behind "IDAT" + data, the Adler-32 sums a, b).
__global__ __launch_bounds__(256) void png_segment_kernel(const ssd_png_desc* __restrict__ desc, const int B, const png_crc_powers P,
                                                         const unsigned char* __restrict__ filtered, unsigned char* __restrict__ slots,
                                                         uint4* __restrict__ meta) {
    __shared__ png_segment S;
    __shared__ unsigned x2n[32];
    const int t = threadIdx.x, g = blockIdx.x;
    const png_seg_place place = png_find_segment(desc, B, g);
    if (t == 0) { S.len = place.len; S.is_first = place.is_first; S.is_last = place.is_last; }
    if (t < 32) x2n[t] = P.x2n[t];
    const uint4* src = reinterpret_cast<const uint4*>(filtered + (long long)g * kPngSeg);
    uint4* in4 = reinterpret_cast<uint4*>(S.in);
    for (int i = t; i < (kPngSeg + 16) / 16; i += kPngThreads) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i * 16 < place.len) v = src[i];
        in4[i] = v;
    }
    png_phase_clear(S, t);
    __syncthreads();
    // the filtered stream's bytes behind the segment's last are another image's or unwritten: zeros, as the host model has them
    for (int i = place.len + t; i < ((place.len + 15) & ~15); i += kPngThreads) S.in[i] = 0;
    __syncthreads();
    png_phase_bounds(S, t);
    __syncthreads();
    png_phase_hist(S, t);
    __syncthreads();
    png_phase_rank_lit(S, t);
    __syncthreads();
    png_phase_plan_lit(S, t);
    __syncthreads();
    png_phase_rank_cl(S, t);
    __syncthreads();
    png_phase_plan_block(S, t);
    __syncthreads();
    png_phase_count(S, t);
    __syncthreads();
    png_phase_write(S, t);
    __syncthreads();
    png_phase_crc(S, t, x2n);
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(slots + (long long)g * kPngSlot);
    const uint4* out4 = reinterpret_cast<const uint4*>(S.out);
    for (int i = t; i * 16 < (int)S.nbytes; i += kPngThreads) dst[i] = out4[i];
    if (t == 0) meta[g] = make_uint4(S.nbytes, png_chunk_crc_register(S, x2n), S.adler_a % kPngAdlerMod, S.adler_b % kPngAdlerMod);
}

// inclusive -> exclusive scan over the kPngScanThreads threads of the one workgroup, through LDS
__device__ __forceinline__ unsigned png_wide_scan(const unsigned v, unsigned* s, unsigned& total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < kPngScanThreads; o <<= 1) {
        const unsigned u = tid >= o ? s[tid - o] : 0u;
        __syncthreads();
        s[tid] += u;
        __syncthreads();
    }
    const unsigned inc = s[tid];
    total = s[kPngScanThreads - 1];
    __syncthreads();
    return inc - v;
}

__device__ __forceinline__ int png_seg_begin(const ssd_png_desc* __restrict__ desc, const int B, const int total, const int b) {
    return b < B ? desc[b].seg_start : total;
}

// Kernel 3: one workgroup.  excl[g]: the bytes of the chunks (12 + data) of the segments before g; a file is the front,
// its chunks, the 4 bytes of Adler-32 inside the last chunk, and IEND.
__global__ __launch_bounds__(1024) void png_scan_kernel(const ssd_png_desc* __restrict__ desc, const int B, const int total,
                                                       const uint4* __restrict__ meta, unsigned* __restrict__ excl, unsigned* __restrict__ adler,
                                                       int* __restrict__ offsets) {
    __shared__ unsigned s[kPngScanThreads];
    const int tid = threadIdx.x;
    {
        const int per = (total + kPngScanThreads - 1) / kPngScanThreads;
        const int lo = min(tid * per, total), hi = min(lo + per, total);
        unsigned sum = 0;
        for (int g = lo; g < hi; ++g) sum += 12u + meta[g].x;
        unsigned all;
        unsigned run = png_wide_scan(sum, s, all);
        for (int g = lo; g < hi; ++g) { excl[g] = run; run += 12u + meta[g].x; }
        if (tid == 0) excl[total] = all;
    }
    __syncthreads();                                                              // excl is read below by other threads of this workgroup
    auto size_of = [&](const int b) {
        return (unsigned)kPngFrontBytes + (excl[png_seg_begin(desc, B, total, b + 1)] - excl[desc[b].seg_start]) + 4u + 12u;
    };
    const int per = (B + kPngScanThreads - 1) / kPngScanThreads;
    const int lo = min(tid * per, B), hi = min(lo + per, B);
    unsigned sum = 0;
    for (int b = lo; b < hi; ++b) {
        sum += size_of(b);
        const ssd_png_desc d = desc[b];
        const long long bytes = png_stream_bytes(d.H, d.W);
        const int end = png_seg_begin(desc, B, total, b + 1);
        unsigned A = 1, Bsum = 0;
        for (int g = d.seg_start; g < end; ++g) {
            const long long left = bytes - (long long)(g - d.seg_start) * kPngSeg;
            const uint4 m = meta[g];
            png_adler_append(A, Bsum, m.z, m.w, (unsigned)(left < kPngSeg ? left : kPngSeg));
        }
        adler[b] = (Bsum << 16) | A;
    }
    unsigned all;
    unsigned run = png_wide_scan(sum, s, all);
    for (int b = lo; b < hi; ++b) { offsets[b] = (int)run; run += size_of(b); }
    if (tid == 0) offsets[B] = (int)all;
}

// Kernel 4: segment g's chunk to its place in file b.
__global__ __launch_bounds__(256) void png_scatter_kernel(const ssd_png_desc* __restrict__ desc, const int B,
                                                         const unsigned char* __restrict__ slots, const uint4* __restrict__ meta,
                                                         const unsigned* __restrict__ excl, const unsigned* __restrict__ adler,
                                                         const int* __restrict__ offsets, unsigned char* __restrict__ out) {
    const int t = threadIdx.x, g = blockIdx.x;
    const png_seg_place place = png_find_segment(desc, B, g);
    const ssd_png_desc d = desc[place.b];
    const uint4 m = meta[g];
    const unsigned n = m.x;
    unsigned char* file = out + offsets[place.b];
    unsigned char* chunk = file + kPngFrontBytes + (excl[g] - excl[d.seg_start]);
    const unsigned char* src = slots + (long long)g * kPngSlot;
    for (unsigned i = t; i < n; i += kPngThreads) chunk[8 + i] = src[i];
    if (t == 0) {
        unsigned crc = m.y;
        unsigned char* tail = chunk + 8 + n;
        png_put_be32(chunk, n + (place.is_last ? 4u : 0u));
        chunk[4] = 'I'; chunk[5] = 'D'; chunk[6] = 'A'; chunk[7] = 'T';
        if (place.is_last) {
            const unsigned a = adler[place.b];
            png_put_be32(tail, a);
            for (int k = 0; k < 4; ++k) crc = png_crc_byte(crc, (a >> (24 - 8 * k)) & 255u);
            tail += 4;
        }
        png_put_be32(tail, ~crc);
        if (place.is_last) png_iend(tail + 4);
    }
    if (t == 64 && place.is_first) png_front(file, d.H, d.W);
}

static const char* const kPngName = "ssd_png_encode";

static bool png_shape_ok(const int H, const int W) { return image_side_ok(H) && image_side_ok(W); }

// One segment through the phases, thread by thread, as the kernel runs them.
static void png_host_segment(png_segment& S, const png_crc_powers& P) {
    auto all = [&](void (*phase)(png_segment&, int)) { for (int t = 0; t < kPngThreads; ++t) phase(S, t); };
    all(png_phase_clear);
    all(png_phase_bounds);
    all(png_phase_hist);
    all(png_phase_rank_lit);
    all(png_phase_plan_lit);
    all(png_phase_rank_cl);
    all(png_phase_plan_block);
    all(png_phase_count);
    all(png_phase_write);
    for (int t = 0; t < kPngThreads; ++t) png_phase_crc(S, t, P.x2n);
}

}  // namespace ssd

using namespace ssd;

extern "C" int ssd_png_segments(int H, int W) { return png_shape_ok(H, W) ? png_segments(H, W) : 0; }

extern "C" size_t ssd_png_encode_bound(int H, int W) { return png_shape_ok(H, W) ? (size_t)png_bound(H, W) : 0; }

extern "C" int ssd_png_encode_host(const unsigned char* rgb, int H, int W, int filter, unsigned char* out, size_t out_bytes, size_t* written) {
    static const char* const name = "ssd_png_encode_host";
    if (written) *written = 0;
    SSD_CHECK_ARG(rgb && out && written, "%s: NULL pointer", name);
    SSD_UNSUPPORTED_IF(!png_shape_ok(H, W), "%s: an image of %d x %d, outside 1..%d", name, H, W, kMaxImageSide);
    SSD_UNSUPPORTED_IF(!png_filter_ok(filter), "%s: filter %d (0..5)", name, filter);
    const png_crc_powers P = png_crc_build_powers();
    const size_t n = 3 * (size_t)W, bytes = (size_t)png_stream_bytes(H, W);
    std::vector<unsigned char> F(bytes);
    for (int y = 0; y < H; ++y) {
        const unsigned char* src = rgb + (size_t)y * n;
        const unsigned char* up = y ? src - n : nullptr;
        auto value = [&](const int type, const size_t x) {
            return png_filter(type, src[x], x >= 3 ? src[x - 3] : 0, up ? up[x] : 0, (up && x >= 3) ? up[x - 3] : 0);
        };
        int type = filter;
        if (type == 5) {
            unsigned sums[5] = {0, 0, 0, 0, 0};
            for (size_t x = 0; x < n; ++x)
                for (int k = 0; k < 5; ++k) sums[k] += png_cost(value(k, x));
            type = png_pick_filter(sums);
        }
        unsigned char* dst = F.data() + (size_t)y * (n + 1);
        dst[0] = (unsigned char)type;
        for (size_t x = 0; x < n; ++x) dst[1 + x] = (unsigned char)value(type, x);
    }
    std::vector<unsigned char> file((size_t)png_bound(H, W));
    std::vector<png_segment> seg(1);
    png_segment& S = seg[0];
    unsigned char* at = file.data();
    png_front(at, H, W);
    at += kPngFrontBytes;
    unsigned A = 1, Bsum = 0;
    const int segs = png_segments(H, W);
    for (int g = 0; g < segs; ++g) {
        const size_t begin = (size_t)g * kPngSeg;
        S.len = (int)(bytes - begin < (size_t)kPngSeg ? bytes - begin : (size_t)kPngSeg);
        S.is_first = g == 0;
        S.is_last = g == segs - 1;
        memset(S.in, 0, sizeof(S.in));
        memcpy(S.in, F.data() + begin, (size_t)S.len);
        png_host_segment(S, P);
        png_adler_append(A, Bsum, S.adler_a, S.adler_b, (unsigned)S.len);
        const unsigned adler = (Bsum << 16) | A, data = S.nbytes + (S.is_last ? 4u : 0u);
        png_put_be32(at, data);
        memcpy(at + 4, "IDAT", 4);
        memcpy(at + 8, S.out, S.nbytes);
        if (S.is_last) png_put_be32(at + 8 + S.nbytes, adler);
        unsigned crc = 0xFFFFFFFFu;                                                 // the plain way: byte by byte over type + data
        for (unsigned i = 4; i < 8 + data; ++i) crc = png_crc_byte(crc, at[i]);
        unsigned pieces = png_chunk_crc_register(S, P.x2n);                         // and as the kernels have it
        if (S.is_last)
            for (int k = 0; k < 4; ++k) pieces = png_crc_byte(pieces, (adler >> (24 - 8 * k)) & 255u);
        if (pieces != crc) {
            set_error("%s: segment %d: the CRC combined from pieces is %08x, byte by byte %08x", name, g, ~pieces, ~crc);
            return SSD_E_STATE;
        }
        png_put_be32(at + 8 + data, ~crc);
        at += 12 + data;
    }
    png_iend(at);
    at += 12;
    const size_t size = (size_t)(at - file.data());
    SSD_CHECK_ARG(out_bytes >= size, "%s: out holds %zu bytes, the file needs %zu", name, out_bytes, size);
    memcpy(out, file.data(), size);
    *written = size;
    return SSD_OK;
}

// the batch's segments, or -1 for a batch no call would take
static long png_total_segments(const ssd_png_desc* desc_host, const int B) {
    long segs = 0;
    for (int b = 0; b < B; ++b) {
        if (!png_shape_ok(desc_host[b].H, desc_host[b].W)) return -1;
        segs += png_segments(desc_host[b].H, desc_host[b].W);
    }
    return segs;
}

extern "C" size_t ssd_png_encode_workspace_bytes(const struct ssd_png_desc* desc_host, int B) {
    if (!desc_host || B <= 0 || B > 65535) return 0;
    const long segs = png_total_segments(desc_host, B);
    return segs < 0 ? 0 : png_layout(segs, B).total;
}

extern "C" int ssd_png_encode(const unsigned char* rgb_dev, size_t rgb_bytes, const struct ssd_png_desc* desc_host,
                              const struct ssd_png_desc* desc_dev, int B, unsigned char* out_dev, size_t out_bytes, int* offsets_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0, "%s: bad batch", kPngName);
    SSD_UNSUPPORTED_IF(B > 65535, "%s: B = %d (at most 65535)", kPngName, B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(rgb_dev && desc_host && desc_dev && out_dev && offsets_dev && workspace_dev, "%s: NULL pointer", kPngName);
    SSD_CHECK_ARG(((size_t)workspace_dev & 15) == 0, "%s: workspace_dev is not 16-byte aligned", kPngName);
    SSD_CHECK_ARG((((size_t)offsets_dev & 3) | ((size_t)desc_dev & 7)) == 0, "%s: offsets_dev / desc_dev are misaligned", kPngName);
    long segs = 0, rows = 0;
    size_t bound = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_png_desc& d = desc_host[b];
        SSD_UNSUPPORTED_IF(!png_shape_ok(d.H, d.W), "%s: image %d is %d x %d, outside 1..%d", kPngName, b, d.H, d.W, kMaxImageSide);
        SSD_UNSUPPORTED_IF(!png_filter_ok(d.filter), "%s: image %d: filter %d (0..5)", kPngName, b, d.filter);
        SSD_CHECK_ARG(region_ok(d.src_offset, (size_t)d.H * d.W * 3, rgb_bytes, 1), "%s: image %d: pixels outside rgb_dev", kPngName, b);
        SSD_CHECK_ARG(d.seg_start == segs && d.row_start == rows, "%s: image %d: seg_start / row_start is not the running sum", kPngName, b);
        segs += png_segments(d.H, d.W);
        rows += d.H;
        bound += (size_t)png_bound(d.H, d.W);
        SSD_UNSUPPORTED_IF(bound > (size_t)INT_MAX, "%s: the files may need more than 2^31 - 1 bytes (image %d)", kPngName, b);
    }
    SSD_CHECK_ARG(out_bytes >= bound, "%s: out holds %zu bytes, the batch may need %zu", kPngName, out_bytes, bound);
    const png_workspace w = png_layout(segs, B);
    SSD_CHECK_ARG(workspace_bytes >= w.total, "%s: the workspace holds %zu bytes, the batch needs %zu", kPngName, workspace_bytes, w.total);
    static const png_crc_powers powers = png_crc_build_powers();
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace_dev;
    unsigned char* filtered = ws + w.filtered;
    unsigned char* slots = ws + w.slots;
    uint4* meta = (uint4*)(ws + w.meta);
    unsigned* excl = (unsigned*)(ws + w.excl);
    unsigned* adler = (unsigned*)(ws + w.adler);
    const int total = (int)segs;
    const dim3 per_row((unsigned)(rows < (1L << 20) ? rows : (1L << 20))), per_seg((unsigned)total), chunk(kPngThreads), one(1), wide(kPngScanThreads);
    hipLaunchKernelGGL(png_filter_kernel, per_row, chunk, 0, st, rgb_dev, desc_dev, B, (int)rows, filtered);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_segment_kernel, per_seg, chunk, 0, st, desc_dev, B, powers, (const unsigned char*)filtered, slots, meta);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_scan_kernel, one, wide, 0, st, desc_dev, B, total, (const uint4*)meta, excl, adler, offsets_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_scatter_kernel, per_seg, chunk, 0, st, desc_dev, B, (const unsigned char*)slots, (const uint4*)meta,
                       (const unsigned*)excl, (const unsigned*)adler, (const int*)offsets_dev, out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
