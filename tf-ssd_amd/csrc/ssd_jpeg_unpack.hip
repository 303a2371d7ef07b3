// The entropy DEcoder on the device ("JPEG decoding: what runs where"): the stuffed scan bytes of a
// ragged batch -> the coefficient storage ssd_jpeg_entropy_decode writes, bit for bit, in the buffer ssd_jpeg_decode reads.
// The decode core and what one thread does in each phase are ssd_jpeg_huff.h (shared with the host model
// ssd_jpeg_entropy_decode_subseq); this file maps the phases to launches.  Four kernels and two fills per call, whatever
// the batch (include/ssd_hip.h spells the contract out):
//   1 zero   every image's coefficient region (one index space of 16-byte pieces over the batch)
//   2 sync   one workgroup per image: its segments' subsequence counts, then the image's subsequences in chunks of 256 --
//            sweeps until no entry state changes, the settled exit of a chunk carried into the next -- and the running
//            sum of the blocks every subsequence completes
//   3 write  one thread per subsequence slot: the settled decode, AC values and DC differences stored, status flags
//   4 dc     one workgroup per image and component: the DC differences summed in scan order, per segment
// No workgroup waits on another.  The segment tables and Huffman tables are device memory the host cannot check: every
// index they produce is clamped or masked, and every store is guarded by the frame.
#include <climits>
#include <cstring>

#include "ssd_jpeg_huff.h"

namespace ssd {

static const char* const kUnpackName = "ssd_jpeg_unpack";

// where the parts of the workspace begin (bytes, each a multiple of 16)
struct unpack_workspace {
    size_t sweeps, nsub, seg_sub, state_p, state_zk, before, total;
};
static unpack_workspace unpack_layout(const long segs, const long slots, const int B) {
    unpack_workspace w;
    size_t at = 0;
    auto part = [&](const size_t bytes) { const size_t here = at; at = align_up(at + bytes, 16); return here; };
    w.sweeps = part((size_t)B * 4); w.nsub = part((size_t)B * 4); w.seg_sub = part((size_t)segs * 4);
    w.state_p = part((size_t)slots * 4); w.state_zk = part((size_t)slots * 4); w.before = part((size_t)slots * 4);
    w.total = at;
    return w;
}

// a multiple of 256 that bounds an image's subsequences (+ 1: the running sum has one entry more): a segment of n bytes
// has max(1, ceil(8 n / S)) <= 8 n / S + 1 of them
static inline long unpack_slots(const long long scan_bytes, const int segments, const int S) {
    const long bound = (long)((scan_bytes * 8 + S - 1) / S) + segments + 1;
    return (bound + kUnpackChunk - 1) / kUnpackChunk * kUnpackChunk;
}

__host__ __device__ __forceinline__ unpack_frame unpack_frame_of(const ssd_jpeg_unpack_desc& d) {
    return unpack_frame_of(d.H, d.W, d.h_samp, d.v_samp, d.components);
}

// exclusive prefix of v over the 256 threads of the workgroup and their total; every thread calls it
__device__ __forceinline__ unsigned unpack_chunk_scan(const unsigned v, unsigned* wave_sums, unsigned& total) {
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
    for (int w = 0; w < kUnpackChunk / 64; ++w) {
        const unsigned s = wave_sums[w];
        if (w < wave) base += s;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

static_assert(sizeof(ssd_jpeg_huff) == 912 && sizeof(ssd_jpeg_segment) == 16 && sizeof(ssd_jpeg_unpack_desc) == 80, "the layouts of include/ssd_hip.h");

struct unpack_lds {
    alignas(16) ssd_jpeg_huff tabs[6];
    unsigned char zz[64];
    unsigned wave[4];
    unsigned exit_p[kUnpackChunk], exit_zk[kUnpackChunk];
};

// kZigzag, four entries a word: handed to the kernels by value, as ssd_jpeg_pack hands its tables
struct unpack_zigzag { unsigned w[16]; };
static unpack_zigzag unpack_zigzag_arg() {
    unpack_zigzag z;
    memset(&z, 0, sizeof(z));
    for (int i = 0; i < 64; ++i) z.w[i >> 2] |= (unsigned)kZigzag[i] << (8 * (i & 3));
    return z;
}

// the image's six tables into LDS, sixteen bytes a load (ssd_jpeg_huff is 912 = 57 x 16 bytes), and kZigzag
__device__ __forceinline__ void unpack_stage_tables(unpack_lds& L, const unsigned char* __restrict__ packed, const ssd_jpeg_unpack_desc& d,
                                                    const unpack_zigzag& zz) {
    const uint4* src = reinterpret_cast<const uint4*>(packed + d.huff_offset);
    uint4* dst = reinterpret_cast<uint4*>(L.tabs);
    for (int i = threadIdx.x; i < (int)(sizeof(L.tabs) / 16); i += kUnpackChunk) dst[i] = src[i];
    if (threadIdx.x < 64) L.zz[threadIdx.x] = (unsigned char)(zz.w[threadIdx.x >> 2] >> (8 * (threadIdx.x & 3)));
}

// the segment that holds subsequence g of the image: the last s with seg_sub[s] <= g (segments clamped to none are skipped)
__device__ __forceinline__ int unpack_find_segment(const unsigned* __restrict__ seg_sub, const int nseg, const unsigned g) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_sub[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// a segment of the image as the kernels take it: inside the image's scan bytes whatever the table holds
__device__ __forceinline__ unpack_seg unpack_load_segment(const unsigned char* __restrict__ packed, const ssd_jpeg_unpack_desc& d, const int s,
                                                          int& first_mcu) {
    const ssd_jpeg_segment t = reinterpret_cast<const ssd_jpeg_segment*>(packed + d.seg_offset)[s];
    const unsigned limit = (unsigned)d.scan_bytes;
    const unsigned first = t.first_byte < limit ? t.first_byte : limit;
    unpack_seg seg = {packed + d.scan_offset + first, t.bytes < limit - first ? t.bytes : limit - first};
    first_mcu = t.first_mcu;
    return seg;
}

__device__ __forceinline__ unsigned unpack_end_bit(const unpack_seg& seg, const unsigned j, const int S) {
    const unsigned long long e = (unsigned long long)(j + 1) * (unsigned)S, all = (unsigned long long)seg.len * 8;
    return (unsigned)(e < all ? e : all);
}

// Kernel 1: zero the images' coefficient regions, and only those.
__global__ __launch_bounds__(256) void jpeg_unpack_zero_kernel(const ssd_jpeg_unpack_desc* __restrict__ desc, const int B, const long total16,
                                                              unsigned char* __restrict__ coef) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total16) return;
    const int blk = (int)(i >> 3);
    const int b = find_image(B, blk, [&](const int k) { return desc[k].block_start; });
    const ssd_jpeg_unpack_desc d = desc[b];
    reinterpret_cast<uint4*>(coef + d.coef_offset)[i - (long)d.block_start * 8] = make_uint4(0u, 0u, 0u, 0u);
}

// Kernel 2: synchronise and place.  Workgroup b owns image b.
__global__ __launch_bounds__(256) void jpeg_unpack_sync_kernel(const unsigned char* __restrict__ packed, const ssd_jpeg_unpack_desc* __restrict__ desc,
                                                              const int S, const unpack_zigzag zz, int* __restrict__ sweeps_out,
                                                              unsigned* __restrict__ nsub_out, unsigned* __restrict__ seg_sub_all,
                                                              unsigned* __restrict__ state_p, unsigned* __restrict__ state_zk,
                                                              unsigned* __restrict__ before, const long total_slots, int* __restrict__ status) {
    __shared__ unpack_lds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const ssd_jpeg_unpack_desc d = desc[b];
    // the image's slots: up to the next image's first, or (the last image) the batch's total
    const unsigned slots = (unsigned)((b + 1 < (int)gridDim.x ? (long)desc[b + 1].sub_start : total_slots) - d.sub_start);
    unpack_stage_tables(L, packed, d, zz);
    const unpack_frame f = unpack_frame_of(d);
    unsigned* seg_sub = seg_sub_all + d.seg_start;
    // every segment's first subsequence: seg_sub[0 .. segments], clamped to the slots the host set aside (a plan's tables
    // never reach the clamp; tables that do are reported)
    unsigned running = 0;
    bool clamped = false;
    for (int s0 = 0; s0 < d.segments; s0 += kUnpackChunk) {
        const int s = s0 + tid;
        unsigned n = 0;
        if (s < d.segments) {
            int first_mcu;
            n = unpack_nsub(unpack_load_segment(packed, d, s, first_mcu).len, S);
        }
        unsigned sum;
        const unsigned excl = unpack_chunk_scan(n, L.wave, sum);
        if (s < d.segments) {
            const unsigned long long at = (unsigned long long)running + excl;
            if (at + n > slots - 1) clamped = true;
            seg_sub[s] = (unsigned)(at < slots - 1 ? at : slots - 1);
        }
        running = (unsigned)((unsigned long long)running + sum < slots - 1 ? running + sum : slots - 1);
    }
    const unsigned nsub = running;
    if (tid == 0) { seg_sub[d.segments] = nsub; nsub_out[b] = nsub; }
    if (clamped) atomicOr(status + b, kUnpackTables);
    __syncthreads();                                                              // seg_sub and the tables are read below

    unsigned done = 0;                                                            // blocks completed before this chunk (wraps with the stream's garbage; differences are what is used)
    int most = 0;
    unsigned* sp = state_p + d.sub_start;
    unsigned* sz = state_zk + d.sub_start;
    unsigned* bf = before + d.sub_start;
    for (unsigned base = 0; base < nsub; base += kUnpackChunk) {
        const unsigned g = base + tid;
        const bool live = g < nsub;
        unpack_seg seg = {packed, 0};
        unpack_state entry = {0, 0, 0};
        unsigned j = 0, end_bit = 0;
        if (live) {
            const int s = unpack_find_segment(seg_sub, d.segments, g);
            int first_mcu;
            seg = unpack_load_segment(packed, d, s, first_mcu);
            j = g - seg_sub[s];
            end_bit = unpack_end_bit(seg, j, S);
            // the segment's first state is known; a chunk's first is the settled exit of the chunk before; the rest guess
            if (j != 0) {
                if (tid == 0) { entry.p = L.exit_p[kUnpackChunk - 1]; entry.z = (int)(L.exit_zk[kUnpackChunk - 1] >> 8); entry.k = (int)(L.exit_zk[kUnpackChunk - 1] & 255); }
                else entry = unpack_guess(seg, j, S);
            }
        }
        __syncthreads();                                                          // the carry has been read
        bool dirty = live;
        unsigned completed = 0;
        int sweep = 0;
        for (; sweep < kUnpackChunk; ++sweep) {
            if (dirty) {
                const unpack_state e = unpack_sweep(seg, L.tabs, f, entry, end_bit, completed);
                L.exit_p[tid] = e.p;
                L.exit_zk[tid] = ((unsigned)e.z << 8) | (unsigned)e.k;
                dirty = false;
            }
            __syncthreads();
            if (live && tid > 0 && j != 0) {                                       // the left neighbour is of the same segment
                const unpack_state e = {L.exit_p[tid - 1], (int)(L.exit_zk[tid - 1] >> 8), (int)(L.exit_zk[tid - 1] & 255)};
                if (e != entry) { entry = e; dirty = true; }
            }
            if (!__syncthreads_or(dirty ? 1 : 0)) break;                           // the vote; it also orders the reads before the next writes
        }
        most = max(most, min(sweep + 1, kUnpackChunk));
        unsigned sum;
        const unsigned excl = unpack_chunk_scan(live ? completed : 0u, L.wave, sum);
        if (live) {
            sp[g] = entry.p;
            sz[g] = ((unsigned)entry.z << 8) | (unsigned)entry.k;
            bf[g] = done + excl;
        }
        done += sum;
    }
    if (tid == 0) { bf[nsub] = done; sweeps_out[b] = most; }
}

// Kernel 3: write.  An image's slots are a multiple of 256, so a workgroup serves one image.
__global__ __launch_bounds__(256) void jpeg_unpack_write_kernel(const unsigned char* __restrict__ packed, const ssd_jpeg_unpack_desc* __restrict__ desc,
                                                               const int B, const int S, const unpack_zigzag zz,
                                                               const unsigned* __restrict__ nsub_in, const unsigned* __restrict__ seg_sub_all,
                                                               const unsigned* __restrict__ state_p, const unsigned* __restrict__ state_zk,
                                                               const unsigned* __restrict__ before, unsigned char* __restrict__ coef,
                                                               int* __restrict__ status) {
    __shared__ unpack_lds L;
    const int first_slot = blockIdx.x * kUnpackChunk;
    const int b = find_image(B, first_slot, [&](const int i) { return desc[i].sub_start; });
    const ssd_jpeg_unpack_desc d = desc[b];
    unpack_stage_tables(L, packed, d, zz);
    __syncthreads();
    const unsigned g = (unsigned)(first_slot - d.sub_start) + threadIdx.x;
    if (g >= nsub_in[b]) return;
    const unpack_frame f = unpack_frame_of(d);
    const unsigned* seg_sub = seg_sub_all + d.seg_start;
    const int s = unpack_find_segment(seg_sub, d.segments, g);
    int first_mcu;
    const unpack_seg seg = unpack_load_segment(packed, d, s, first_mcu);
    const unsigned first = seg_sub[s], j = g - first;
    const unsigned* bf = before + d.sub_start;
    const unpack_state st = {state_p[d.sub_start + g], (int)(state_zk[d.sub_start + g] >> 8), (int)(state_zk[d.sub_start + g] & 255)};
    const long ri = d.restart_interval, left = (long)f.mcus - first_mcu;
    const long seg_mcus = first_mcu < 0 || left <= 0 ? 0 : (ri > 0 && ri < left ? ri : left);
    const int flags = unpack_write(seg, L.tabs, f, L.zz, st, unpack_end_bit(seg, j, S), bf[g] - bf[first], (unsigned)(seg_mcus * f.nz), first_mcu,
                                   g + 1 == seg_sub[s + 1], s + 1 == d.segments, reinterpret_cast<short*>(coef + d.coef_offset));
    if (flags) atomicOr(status + b, flags);
}

// Kernel 4: DC prediction.  Workgroup (b, c) walks component c's DC differences in SCAN order (MCU order, not plane raster
// order) in chunks of 256 and replaces each with the sum of its segment so far.  decode_block computes coef[0] =
// (short)(unsigned 32-bit running sum), so a sum that wraps -- at 32 bits here, at 16 just as well -- gives the same bits.
// A segment restarts the sum: with P the running sum over the whole component, the answer is P[e] - P[first of e's
// segment - 1], which needs no segmented scan.
__global__ __launch_bounds__(256) void jpeg_unpack_dc_kernel(const ssd_jpeg_unpack_desc* __restrict__ desc, unsigned char* __restrict__ coef_all) {
    __shared__ unsigned wave[4];
    __shared__ unsigned incl[kUnpackChunk];
    const int b = blockIdx.x / 3, c = blockIdx.x - b * 3, tid = threadIdx.x;
    const ssd_jpeg_unpack_desc d = desc[b];
    if (c >= d.components) return;
    const unpack_frame f = unpack_frame_of(d);
    short* coef = reinterpret_cast<short*>(coef_all + d.coef_offset);
    const int per = c == 0 ? f.nl : 1;
    const long total = (long)f.mcus * per;
    const long seglen = d.restart_interval > 0 ? (long)d.restart_interval * per : total;
    unsigned carry = 0, segbase = 0;              // P before this chunk; P before the segment that holds the chunk's first element
    for (long base = 0; base < total; base += kUnpackChunk) {
        const long e = base + tid;
        const bool live = e < total;
        long at = 0;
        unsigned v = 0;
        if (live) {
            at = unpack_dc_at(f, c, per, (int)e);
            v = (unsigned)(int)coef[at];
        }
        unsigned sum;
        const unsigned p = carry + unpack_chunk_scan(v, wave, sum) + v;
        incl[tid] = p;
        __syncthreads();
        if (live) {
            const long ss = e / seglen * seglen;                                   // the first element of e's segment
            const unsigned sub = ss > base ? incl[ss - 1 - base] : (ss == 0 ? 0u : segbase);
            coef[at] = (short)(p - sub);
        }
        const long nb = base + kUnpackChunk, ssn = nb / seglen * seglen;
        if (ssn > base) segbase = incl[ssn - 1 - base];                            // ssn - 1 < nb: inside this chunk
        carry += sum;
        __syncthreads();
    }
}

}  // namespace ssd

using namespace ssd;

static inline bool unpack_desc_ok(const ssd_jpeg_unpack_desc& d) {
    if (!image_side_ok(d.H) || !image_side_ok(d.W)) return false;
    if (d.components == 1) return d.h_samp == 1 && d.v_samp == 1;
    return d.components == 3 && jpeg_sampling_ok(d.h_samp, d.v_samp);
}
static inline bool unpack_bits_ok(const int S) { return S % 32 == 0 && S >= 128 && S <= SSD_JPEG_UNPACK_MAX_SUBSEQ_BITS; }

extern "C" int ssd_jpeg_unpack_slots(long long scan_bytes, int segments, int subseq_bits) {
    const int S = subseq_bits ? subseq_bits : kUnpackDefaultBits;
    if (!unpack_bits_ok(S) || scan_bytes < 0 || scan_bytes >= SSD_JPEG_UNPACK_MAX_SCAN_BYTES || segments < 1) return 0;
    const long n = unpack_slots(scan_bytes, segments, S);
    return n < INT_MAX ? (int)n : 0;
}

extern "C" size_t ssd_jpeg_unpack_workspace_bytes(const struct ssd_jpeg_unpack_desc* desc_host, int B, int subseq_bits) {
    if (!desc_host || B <= 0 || B > 65535) return 0;
    long segs = 0, slots = 0;
    for (int b = 0; b < B; ++b) {
        const int n = ssd_jpeg_unpack_slots(desc_host[b].scan_bytes, desc_host[b].segments, subseq_bits);
        if (n == 0) return 0;
        segs += (long)desc_host[b].segments + 1;
        slots += n;
    }
    return unpack_layout(segs, slots, B).total;
}

extern "C" int ssd_jpeg_unpack(const unsigned char* packed_dev, size_t packed_bytes, const struct ssd_jpeg_unpack_desc* desc_host,
                               const struct ssd_jpeg_unpack_desc* desc_dev, int B, int subseq_bits, unsigned char* coef_dev,
                               size_t coef_bytes, int* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0, "%s: bad batch", kUnpackName);
    SSD_UNSUPPORTED_IF(B > 65535, "%s: B = %d (at most 65535)", kUnpackName, B);
    if (B == 0) return SSD_OK;
    const int S = subseq_bits ? subseq_bits : kUnpackDefaultBits;
    SSD_UNSUPPORTED_IF(!unpack_bits_ok(S), "%s: subseq_bits = %d (0, or a multiple of 32 in 128..%d)", kUnpackName, subseq_bits,
                       SSD_JPEG_UNPACK_MAX_SUBSEQ_BITS);
    SSD_CHECK_ARG(packed_dev && desc_host && desc_dev && coef_dev && status_dev && workspace_dev, "%s: NULL pointer", kUnpackName);
    SSD_CHECK_ARG((((size_t)packed_dev | (size_t)coef_dev | (size_t)workspace_dev) & 15) == 0, "%s: a buffer is not 16-byte aligned", kUnpackName);
    SSD_CHECK_ARG(((size_t)status_dev & 3) == 0, "%s: status_dev is not 4-byte aligned", kUnpackName);
    SSD_CHECK_ARG((size_t)coef_dev + coef_bytes <= (size_t)packed_dev || (size_t)packed_dev + packed_bytes <= (size_t)coef_dev,
                  "%s: coef_dev overlaps packed_dev", kUnpackName);
    long blocks = 0, segs = 0, slots = 0;
    size_t coef_end = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_unpack_desc& d = desc_host[b];
        SSD_UNSUPPORTED_IF(!image_side_ok(d.H) || !image_side_ok(d.W), "%s: image %d is %d x %d, outside 1..%d", kUnpackName, b, d.H, d.W,
                           kMaxImageSide);
        SSD_UNSUPPORTED_IF(!unpack_desc_ok(d), "%s: image %d: %d components sampled %dx%d", kUnpackName, b, d.components, d.h_samp, d.v_samp);
        SSD_CHECK_ARG(d.scan_bytes >= 0, "%s: image %d: negative scan_bytes", kUnpackName, b);
        SSD_UNSUPPORTED_IF(d.scan_bytes >= SSD_JPEG_UNPACK_MAX_SCAN_BYTES, "%s: image %d: %lld bytes of entropy-coded data (below %lld only)",
                           kUnpackName, b, d.scan_bytes, (long long)SSD_JPEG_UNPACK_MAX_SCAN_BYTES);
        const unpack_frame f = unpack_frame_of(d);
        SSD_CHECK_ARG(d.restart_interval >= 0 && d.restart_interval <= 65535, "%s: image %d: restart interval %d", kUnpackName, b, d.restart_interval);
        const int need = d.restart_interval ? (f.mcus + d.restart_interval - 1) / d.restart_interval : 1;
        SSD_CHECK_ARG(d.segments == need, "%s: image %d: %d segments, the frame has %d", kUnpackName, b, d.segments, need);
        SSD_CHECK_ARG(region_ok(d.scan_offset, (size_t)d.scan_bytes, packed_bytes, 16), "%s: image %d: scan bytes outside packed_dev or misaligned",
                      kUnpackName, b);
        SSD_CHECK_ARG(region_ok(d.huff_offset, 6 * sizeof(ssd_jpeg_huff), packed_bytes, 16),
                      "%s: image %d: Huffman tables outside packed_dev or misaligned", kUnpackName, b);
        SSD_CHECK_ARG(region_ok(d.seg_offset, (size_t)d.segments * sizeof(ssd_jpeg_segment), packed_bytes, 16),
                      "%s: image %d: segment table outside packed_dev or misaligned", kUnpackName, b);
        SSD_CHECK_ARG(region_ok(d.coef_offset, (size_t)f.g.nblocks * 128, coef_bytes, 16, &coef_end),
                      "%s: image %d: coefficients outside coef_dev, misaligned or overlapping", kUnpackName, b);
        SSD_CHECK_ARG(d.block_start == blocks && d.seg_start == segs && d.sub_start == slots,
                      "%s: image %d: block_start / seg_start / sub_start are not the running sums", kUnpackName, b);
        blocks += f.g.nblocks;
        segs += (long)d.segments + 1;
        slots += unpack_slots(d.scan_bytes, d.segments, S);
        SSD_UNSUPPORTED_IF(blocks >= (1L << 31) - 64 || slots >= (1L << 31) - 512 || segs >= (1L << 31) - 512,
                           "%s: the batch is too large for one call (image %d)", kUnpackName, b);
    }
    const unpack_workspace w = unpack_layout(segs, slots, B);
    SSD_CHECK_ARG(workspace_bytes >= w.total, "%s: the workspace holds %zu bytes, the batch needs %zu", kUnpackName, workspace_bytes, w.total);
    static const unpack_zigzag zz = unpack_zigzag_arg();
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace_dev;
    int* sweeps = (int*)(ws + w.sweeps);
    unsigned* nsub = (unsigned*)(ws + w.nsub);
    unsigned* seg_sub = (unsigned*)(ws + w.seg_sub);
    unsigned* state_p = (unsigned*)(ws + w.state_p);
    unsigned* state_zk = (unsigned*)(ws + w.state_zk);
    unsigned* before = (unsigned*)(ws + w.before);
    SSD_HIP(hipMemsetAsync(ws, 0, w.total, st));
    SSD_HIP(hipMemsetAsync(status_dev, 0, (size_t)B * 4, st));
    const long total16 = blocks * 8;
    hipLaunchKernelGGL(jpeg_unpack_zero_kernel, dim3((unsigned)((total16 + 255) / 256)), dim3(256), 0, st, desc_dev, B, total16, coef_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_unpack_sync_kernel, dim3((unsigned)B), dim3(kUnpackChunk), 0, st, packed_dev, desc_dev, S, zz, sweeps, nsub, seg_sub,
                       state_p, state_zk, before, slots, status_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_unpack_write_kernel, dim3((unsigned)(slots / kUnpackChunk)), dim3(kUnpackChunk), 0, st, packed_dev, desc_dev, B, S, zz,
                       (const unsigned*)nsub, (const unsigned*)seg_sub, (const unsigned*)state_p, (const unsigned*)state_zk,
                       (const unsigned*)before, coef_dev, status_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_unpack_dc_kernel, dim3((unsigned)B * 3), dim3(kUnpackChunk), 0, st, desc_dev, coef_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
