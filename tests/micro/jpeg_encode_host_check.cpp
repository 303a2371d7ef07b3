// Stand-alone check of the JPEG encoder's and decoder's host halves under a sanitizer (CPU only; never loaded into Python, needs no GPU).
// Links csrc/ssd_jpeg_enc.hip and csrc/ssd_jpeg.hip with an error sink of its own and reads the cases
// tests/micro/jpeg_encode_host_check.sh dumps from the fixture: per case H, W, h_samp, v_samp, quality (int32), the int16
// coefficient storage of the NumPy restatement and the bytes Pillow wrote.  Every buffer handed to the library is a heap
// block of exactly the size it is told, so a read or write outside it is an AddressSanitizer report.
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

int main(int argc, char** argv) {
    FILE* f = fopen(argc > 1 ? argv[1] : "jpeg_encode_cases.bin", "rb");
    if (!f) { perror("cases"); return 2; }
    int n = 0, head[7];
    while (fread(head, sizeof(int), 7, f) == 7) {
        const int H = head[0], W = head[1], hs = head[2], vs = head[3], quality = head[4];
        std::vector<short> coef((size_t)head[5]);
        std::vector<unsigned char> want((size_t)head[6]);
        REQUIRE(fread(coef.data(), 2, coef.size(), f) == coef.size() && fread(want.data(), 1, want.size(), f) == want.size());
        unsigned short tables[128];
        ssd_jpeg_info info;
        REQUIRE(ssd_jpeg_quality_tables(quality, tables) == SSD_OK);
        REQUIRE(ssd_jpeg_encode_info(W, H, hs, vs, tables, &info) == SSD_OK);
        REQUIRE((size_t)info.coef_bytes == coef.size() * 2);
        const size_t bound = ssd_jpeg_encode_bound(&info);
        REQUIRE(bound >= want.size());
        size_t written = 0;
        for (const size_t room : {bound, want.size()}) {                              // the bound, and exactly enough
            std::vector<unsigned char> out(room);
            REQUIRE(ssd_jpeg_entropy_encode(coef.data(), &info, out.data(), out.size(), &written) == SSD_OK);
            REQUIRE(written == want.size() && memcmp(out.data(), want.data(), written) == 0);
        }
        for (const size_t room : {want.size() - 1, want.size() / 2, (size_t)300, (size_t)1}) {      // too small
            std::vector<unsigned char> out(room);
            REQUIRE(ssd_jpeg_entropy_encode(coef.data(), &info, out.data(), out.size(), &written) == SSD_E_INVALID);
        }
        ssd_jpeg_info bad = info;
        bad.mcus_x += 1;                                                               // a damaged info reads nothing
        std::vector<unsigned char> out(bound);
        REQUIRE(ssd_jpeg_entropy_encode(coef.data(), &bad, out.data(), out.size(), &written) == SSD_E_INVALID);
        std::vector<short> wild(coef);                                                 // out-of-range values: an error, no UB
        wild[0] = 32767; wild[1] = -32768;
        REQUIRE(ssd_jpeg_entropy_encode(wild.data(), &info, out.data(), out.size(), &written) == SSD_E_INVALID);
        // the decoder's host half on the same stream: the frame it parses is the case's, its struct ssd_jpeg_info is the
        // encoder's byte for byte (both complete it with the same code), and it decodes into a block of exactly coef_bytes
        ssd_jpeg_info parsed;
        REQUIRE(ssd_jpeg_parse(want.data(), want.size(), &parsed) == SSD_OK);
        REQUIRE(parsed.width == W && parsed.height == H && parsed.components == 3);
        REQUIRE(parsed.h_samp[0] == hs && parsed.v_samp[0] == vs);
        for (int c = 1; c < 3; ++c) REQUIRE(parsed.h_samp[c] == 1 && parsed.v_samp[c] == 1);
        REQUIRE(memcmp(&parsed, &info, sizeof(info)) == 0);
        std::vector<short> back(coef.size());
        REQUIRE(ssd_jpeg_entropy_decode(want.data(), want.size(), &parsed, back.data(), back.size() * 2) == SSD_OK);
        REQUIRE(back[0] == coef[0]);                                                   // the first luma DC term, at least
        std::vector<short> small(coef.size() - 64);                                    // one block short: refused, not overrun
        REQUIRE(ssd_jpeg_entropy_decode(want.data(), want.size(), &parsed, small.data(), small.size() * 2) == SSD_E_INVALID);
        REQUIRE(ssd_jpeg_entropy_decode(want.data(), want.size() / 2, &parsed, back.data(), back.size() * 2) == SSD_E_INVALID);
        ++n;
    }
    fclose(f);
    printf("%d cases: bytes equal, parsed back to the same frame, nothing outside the buffers\n", n);
    return n > 0 ? 0 : 3;
}
