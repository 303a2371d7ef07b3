// Stand-alone check of the PNG encoder's host model under a sanitizer (CPU only; never loaded into Python, needs no GPU).
// Links csrc/ssd_png.hip with an error sink of its own and reads the cases tests/micro/png_host_check.sh dumps from
// tests/png_cases.py: per case H, W, filter, the size of the restated filtered stream (int32), the pixels and that stream.
// Every buffer handed to the library is a heap block of exactly the size it is told, so a read or write outside it is an
// AddressSanitizer report.  The file is taken apart here with nothing from the library: chunk walk with a bytewise CRC-32,
// and an inflate that knows the three block types, whose output must be the restated stream and match the Adler-32.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/ssd_hip.h"

namespace ssd {
void set_error(const char* fmt, ...) {
    static thread_local char text[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof(text), fmt, ap);
    va_end(ap);
}
}  // namespace ssd

#define REQUIRE(cond)                                                                   \
    do {                                                                                \
        if (!(cond)) { fprintf(stderr, "case %d: %s failed (line %d)\n", n, #cond, __LINE__); return 1; } \
    } while (0)

static unsigned crc32_of(const unsigned char* p, size_t len) {
    unsigned crc = 0xFFFFFFFFu;
    for (size_t i = 0; i < len; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ ((crc & 1u) ? 0xEDB88320u : 0u);
    }
    return ~crc;
}
static unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }

// a small strict inflate: false on anything RFC 1951 does not allow
struct bit_reader {
    const std::vector<unsigned char>& d;
    size_t at = 0;
    bool ok = true;
    explicit bit_reader(const std::vector<unsigned char>& data) : d(data) {}
    unsigned take(int bits) {
        unsigned v = 0;
        for (int i = 0; i < bits; ++i, ++at) {
            if (at >> 3 >= d.size()) { ok = false; return 0; }
            v |= (unsigned)((d[at >> 3] >> (at & 7)) & 1) << i;
        }
        return v;
    }
};
struct huffman {
    int count[16] = {0};
    std::vector<int> symbol;
    bool build(const std::vector<int>& len, bool allow_one) {
        int used = 0;
        for (int l : len) { ++count[l]; used += l ? 1 : 0; }
        count[0] = 0;
        long left = 1;
        for (int l = 1; l < 16; ++l) { left = 2 * left - count[l]; if (left < 0) return false; }
        if (left != 0 && !(allow_one && used == 1 && count[1] == 1)) return false;      // complete, or the single one-bit code
        int offs[16] = {0};
        for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + count[l];
        symbol.assign(len.size(), 0);
        for (size_t s = 0; s < len.size(); ++s)
            if (len[s]) symbol[offs[len[s]]++] = (int)s;
        return true;
    }
    int decode(bit_reader& r) const {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l < 16; ++l) {
            code |= (int)r.take(1);
            if (!r.ok) return -1;
            if (code - count[l] < first) return symbol[index + (code - first)];
            index += count[l]; first += count[l]; first <<= 1; code <<= 1;
        }
        return -1;
    }
};
static bool inflate_all(const std::vector<unsigned char>& data, std::vector<unsigned char>& out) {
    static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    bit_reader r(data);
    for (;;) {
        const unsigned final = r.take(1), type = r.take(2);
        if (!r.ok || type == 3 || type == 1) return false;                            // the encoder never writes fixed blocks
        if (type == 0) {
            r.at = (r.at + 7) & ~(size_t)7;
            const unsigned len = r.take(16), nlen = r.take(16);
            if (!r.ok || (len ^ nlen) != 0xFFFFu) return false;
            for (unsigned i = 0; i < len; ++i) { out.push_back((unsigned char)r.take(8)); if (!r.ok) return false; }
        } else {
            const int hlit = (int)r.take(5) + 257, hdist = (int)r.take(5) + 1, hclen = (int)r.take(4) + 4;
            if (hlit > 286) return false;
            std::vector<int> cl(19, 0);
            for (int i = 0; i < hclen; ++i) cl[order[i]] = (int)r.take(3);
            huffman clh;
            if (!clh.build(cl, false)) return false;
            std::vector<int> len;
            while ((int)len.size() < hlit + hdist) {
                const int s = clh.decode(r);
                if (s < 0) return false;
                if (s < 16) len.push_back(s);
                else if (s == 16) { if (len.empty()) return false; const int v = len.back(); for (int k = (int)r.take(2) + 3; k > 0; --k) len.push_back(v); }
                else for (int k = s == 17 ? (int)r.take(3) + 3 : (int)r.take(7) + 11; k > 0; --k) len.push_back(0);
            }
            if ((int)len.size() != hlit + hdist || len[256] == 0) return false;
            huffman lit, dist;
            if (!lit.build(std::vector<int>(len.begin(), len.begin() + hlit), false)) return false;
            if (!dist.build(std::vector<int>(len.begin() + hlit, len.end()), true)) return false;
            for (;;) {
                const int s = lit.decode(r);
                if (s < 0) return false;
                if (s < 256) { out.push_back((unsigned char)s); continue; }
                if (s == 256) break;
                const int l = lbase[s - 257] + (int)r.take(lext[s - 257]);
                const int d = dist.decode(r);
                if (d != 0 || out.empty()) return false;                              // distance 1 only
                const unsigned char v = out.back();
                for (int k = 0; k < l; ++k) out.push_back(v);
            }
        }
        if (final) break;
    }
    return r.ok && ((r.at + 7) >> 3) == data.size() - 4;                             // the Adler-32 follows the last block's byte
}

int main(int argc, char** argv) {
    FILE* f = fopen(argc > 1 ? argv[1] : "png_cases.bin", "rb");
    if (!f) { perror("cases"); return 2; }
    int n = 0, head[4];
    while (fread(head, sizeof(int), 4, f) == 4) {
        const int H = head[0], W = head[1], filter = head[2];
        std::vector<unsigned char> rgb((size_t)H * W * 3), want((size_t)head[3]);
        REQUIRE(fread(rgb.data(), 1, rgb.size(), f) == rgb.size() && fread(want.data(), 1, want.size(), f) == want.size());
        const size_t bound = ssd_png_encode_bound(H, W);
        const int segments = ssd_png_segments(H, W);
        REQUIRE(bound == 45 + 17 * (size_t)segments + want.size() + 6 && (size_t)segments == (want.size() + 16383) / 16384);
        std::vector<unsigned char> file(bound);
        size_t written = 0;
        REQUIRE(ssd_png_encode_host(rgb.data(), H, W, filter, file.data(), file.size(), &written) == SSD_OK);
        REQUIRE(written >= 57 && written <= bound);
        file.resize(written);
        {                                                                             // exactly enough; one byte short
            std::vector<unsigned char> exact(written), small(written - 1, 0x5A);
            size_t w2 = 0;
            REQUIRE(ssd_png_encode_host(rgb.data(), H, W, filter, exact.data(), exact.size(), &w2) == SSD_OK && w2 == written);
            REQUIRE(memcmp(exact.data(), file.data(), written) == 0);
            REQUIRE(ssd_png_encode_host(rgb.data(), H, W, filter, small.data(), small.size(), &w2) == SSD_E_INVALID && w2 == 0);
            for (unsigned char v : small) REQUIRE(v == 0x5A);
        }
        static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
        REQUIRE(memcmp(file.data(), sig, 8) == 0);
        size_t at = 8;
        int chunks = 0, idats = 0;
        std::vector<unsigned char> z;
        bool ended = false;
        while (at < file.size()) {
            REQUIRE(!ended && at + 12 <= file.size());
            const unsigned len = be32(&file[at]);
            REQUIRE(at + 12 + len <= file.size());
            REQUIRE(be32(&file[at + 8 + len]) == crc32_of(&file[at + 4], 4 + len));
            if (chunks == 0) {
                REQUIRE(memcmp(&file[at + 4], "IHDR", 4) == 0 && len == 13);
                REQUIRE(be32(&file[at + 8]) == (unsigned)W && be32(&file[at + 12]) == (unsigned)H);
                REQUIRE(file[at + 16] == 8 && file[at + 17] == 2 && file[at + 18] == 0 && file[at + 19] == 0 && file[at + 20] == 0);
            } else if (memcmp(&file[at + 4], "IDAT", 4) == 0) {
                ++idats;
                z.insert(z.end(), file.begin() + at + 8, file.begin() + at + 8 + len);
            } else {
                REQUIRE(memcmp(&file[at + 4], "IEND", 4) == 0 && len == 0);
                ended = true;
            }
            ++chunks;
            at += 12 + len;
        }
        REQUIRE(ended && idats == segments && chunks == segments + 2);
        REQUIRE(z.size() >= 6 && z[0] == 0x78 && z[1] == 0x9C);
        std::vector<unsigned char> deflate(z.begin() + 2, z.end()), back;
        REQUIRE(inflate_all(deflate, back));
        REQUIRE(back == want);
        unsigned a = 1, b = 0;
        for (unsigned char v : back) { a = (a + v) % 65521u; b = (b + a) % 65521u; }
        REQUIRE(be32(&z[z.size() - 4]) == ((b << 16) | a));
        ++n;
    }
    fclose(f);
    unsigned char px[3] = {1, 2, 3}, out[128];
    size_t written = 9;
    if (ssd_png_encode_host(nullptr, 1, 1, 5, out, sizeof(out), &written) != SSD_E_INVALID || written != 0 ||
        ssd_png_encode_host(px, 1, 1, 6, out, sizeof(out), &written) != SSD_E_UNSUPPORTED ||
        ssd_png_encode_host(px, 0, 1, 5, out, sizeof(out), &written) != SSD_E_UNSUPPORTED) {
        fprintf(stderr, "refusals failed\n");
        return 1;
    }
    printf("%d cases: every chunk's CRC, the inflated stream and its Adler-32 as restated, nothing outside the buffers\n", n);
    return n > 0 ? 0 : 3;
}
