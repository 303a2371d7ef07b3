// PNG inflate on the device ("PNG inflate on the device"; the contract: include/ssd_hip.h, "PNG
// INFLATE").  Two kernels per call, whatever the batch:
//   1 inflate  one wavefront (one workgroup of 64) per zlib stream runs png_inflate_stream<64> (ssd_png_inflate.h): the
//              decode state is the same in every lane, the window, the staged input and the code tables live in LDS.
//   2 chains   one workgroup per image turns the H filter bytes into the chain list ssd_png_decode reads, padded with H.
// ssd_png_inflate_host runs png_inflate_stream<1> and the same filter rule as plain loops.  Integer arithmetic only.
#include <algorithm>
#include <memory>
#include <vector>

#include "ssd_png_inflate.h"

namespace ssd {

static const int kInfChainThreads = 256;

__global__ __launch_bounds__(64) void png_inflate_kernel(unsigned char* packed, const ssd_png_inflate_desc* __restrict__ desc, int* __restrict__ status) {
    __shared__ png_inf_work w;
    const ssd_png_inflate_desc d = desc[blockIdx.x];
    const unsigned st = png_inflate_stream<64>(w, packed + d.zlib_offset, d.zlib_bytes, packed + d.dst_offset, (long long)d.H * (1 + d.row_bytes),
                                               (int)threadIdx.x);
    if (threadIdx.x == 0) status[blockIdx.x] = (int)st;
}

// Image blockIdx.x: rows 0 and those of filter type 0 or 1, ascending, then H in every slot that is left.
__global__ __launch_bounds__(kInfChainThreads) void png_chain_kernel(unsigned char* packed, const ssd_png_inflate_desc* __restrict__ desc,
                                                                    int* __restrict__ status) {
    __shared__ int wave_count[kInfChainThreads / 64];
    __shared__ int bad;
    const ssd_png_inflate_desc d = desc[blockIdx.x];
    const unsigned char* rows = packed + d.dst_offset;
    int* list = reinterpret_cast<int*>(packed + d.chain_offset);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool inflated = status[blockIdx.x] == 0;          // else the bytes are unspecified: their filter bytes say nothing
    if (tid == 0) bad = 0;
    int found = 0;                                          // chains before this tile
    for (int y0 = 0; y0 < d.H; y0 += kInfChainThreads) {
        const int y = y0 + tid;
        const int type = y < d.H ? rows[(long long)y * (1 + d.row_bytes)] : 2;
        const bool starts = y < d.H && (y == 0 || type <= 1);
        const unsigned long long mask = __ballot(starts);
        __syncthreads();                                    // the tile before has read wave_count
        if (lane == 0) wave_count[wave] = __popcll(mask);
        if (type > 4) bad = 1;
        __syncthreads();
        int before = found;
        for (int k = 0; k < wave; ++k) before += wave_count[k];
        if (starts) list[before + __popcll(mask & ((1ull << lane) - 1ull))] = y;
        for (int k = 0; k < kInfChainThreads / 64; ++k) found += wave_count[k];
    }
    __syncthreads();
    for (int k = found + tid; k < d.H; k += kInfChainThreads) list[k] = d.H;
    if (tid == 0 && bad && inflated) status[blockIdx.x] = SSD_PNG_INFLATE_FILTER;
}

static const char* const kPngInfName = "ssd_png_inflate";

}  // namespace ssd

using namespace ssd;

extern "C" int ssd_png_inflate_host(const unsigned char* zlib, size_t n, unsigned char* out, size_t out_bytes, long long row_bytes, int* status) {
    static const char* const name = "ssd_png_inflate_host";
    SSD_CHECK_ARG(zlib && out && status, "%s: NULL pointer", name);
    SSD_CHECK_ARG(row_bytes >= 1 && out_bytes >= 1 && out_bytes % (size_t)(1 + row_bytes) == 0, "%s: %zu bytes are no rows of 1 + %lld", name, out_bytes,
                  row_bytes);
    std::unique_ptr<png_inf_work> w(new png_inf_work);
    unsigned st = png_inflate_stream<1>(*w, zlib, (long long)n, out, (long long)out_bytes, 0);
    if (st == 0) {
        for (size_t at = 0; at < out_bytes; at += (size_t)(1 + row_bytes))
            if (out[at] > 4) st = SSD_PNG_INFLATE_FILTER;
    }
    *status = (int)st;
    return SSD_OK;
}

extern "C" int ssd_png_inflate(unsigned char* packed_dev, size_t packed_bytes, const struct ssd_png_inflate_desc* desc_host,
                               const struct ssd_png_inflate_desc* desc_dev, int B, int* status_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0, "%s: bad batch", kPngInfName);
    SSD_UNSUPPORTED_IF(B > 65535, "%s: B = %d (at most 65535)", kPngInfName, B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(packed_dev && desc_host && desc_dev && status_dev, "%s: NULL pointer", kPngInfName);
    SSD_CHECK_ARG(((size_t)packed_dev & 15) == 0 && ((size_t)desc_dev & 7) == 0 && ((size_t)status_dev & 3) == 0,
                  "%s: packed_dev is not 16-byte aligned, desc_dev not 8-byte or status_dev not 4-byte", kPngInfName);
    std::vector<std::pair<size_t, size_t>> regions;        // (begin, end) of everything the batch reads or writes in packed_dev
    regions.reserve(3 * (size_t)B);
    for (int b = 0; b < B; ++b) {
        const ssd_png_inflate_desc& d = desc_host[b];
        SSD_CHECK_ARG(d.H >= 1 && d.row_bytes >= 1 && d.zlib_bytes >= 0 && d.reserved == 0, "%s: image %d: H = %d, row_bytes = %lld, zlib_bytes = %lld, reserved = %d",
                      kPngInfName, b, d.H, d.row_bytes, d.zlib_bytes, d.reserved);
        SSD_UNSUPPORTED_IF(d.row_bytes >= kInfMaxStream || (long long)d.H * (1 + d.row_bytes) > kInfMaxStream,
                           "%s: image %d: a stream of %d x (1 + %lld) bytes, above %lld", kPngInfName, b, d.H, d.row_bytes, kInfMaxStream);
        const size_t out = (size_t)d.H * (size_t)(1 + d.row_bytes);
        SSD_CHECK_ARG((size_t)d.zlib_bytes <= packed_bytes && region_ok(d.zlib_offset, (size_t)d.zlib_bytes, packed_bytes, 16) &&
                          region_ok(d.dst_offset, out, packed_bytes, 16) && region_ok(d.chain_offset, 4 * (size_t)d.H, packed_bytes, 16),
                      "%s: image %d: a region misaligned or outside packed_dev", kPngInfName, b);
        regions.emplace_back((size_t)d.zlib_offset, (size_t)d.zlib_offset + (size_t)d.zlib_bytes);
        regions.emplace_back((size_t)d.dst_offset, (size_t)d.dst_offset + out);
        regions.emplace_back((size_t)d.chain_offset, (size_t)d.chain_offset + 4 * (size_t)d.H);
    }
    std::sort(regions.begin(), regions.end());
    for (size_t i = 1; i < regions.size(); ++i)
        SSD_CHECK_ARG(regions[i].first >= regions[i - 1].second, "%s: two regions of the batch overlap at byte %zu of packed_dev", kPngInfName, regions[i].first);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)B), dim3(64), 0, st, packed_dev, desc_dev, status_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_chain_kernel, dim3((unsigned)B), dim3(kInfChainThreads), 0, st, packed_dev, desc_dev, status_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
