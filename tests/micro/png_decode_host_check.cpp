// Stand-alone check of the PNG decoder's host half and host model under a sanitizer (CPU only; never loaded into Python,
// needs no GPU).  Links csrc/ssd_png_dec.hip with an error sink of its own and reads the cases
// tests/micro/png_decode_host_check.sh dumps from tests/png_decode_cases.py: per case five int32 -- the file's size, the
// size of the inflated stream, H, W, the code ssd_png_parse must answer -- then the file, the stream and Pillow's pixels
// (the last two only where the code is 0 and the stream is the image's).  Every buffer handed to the library is a heap
// block of exactly the size it is told, so a read or write outside it is an AddressSanitizer report.  Then every
// truncation and every single-byte corruption of the first three files goes through ssd_png_parse and, where that
// accepts, ssd_png_idat: any answer is fine, any report is not.
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

// the file as a heap block of its own size
static int parse_exact(const std::vector<unsigned char>& file, ssd_png_info* info) {
    unsigned char* block = new unsigned char[file.size() ? file.size() : 1];
    if (!file.empty()) memcpy(block, file.data(), file.size());
    int rc = ssd_png_parse(block, file.size(), info);
    if (rc == SSD_OK) {
        unsigned char* stream = new unsigned char[info->idat_bytes ? info->idat_bytes : 1];
        rc = ssd_png_idat(block, file.size(), info, stream, (size_t)info->idat_bytes);
        delete[] stream;
    }
    delete[] block;
    return rc;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0, decoded = 0;
    long mangled = 0, still_accepted = 0;
    int head[5];
    while (fread(head, sizeof(int), 5, f) == 5) {
        const int file_bytes = head[0], stream_bytes = head[1], H = head[2], W = head[3], code = head[4];
        std::vector<unsigned char> file((size_t)file_bytes);
        REQUIRE(fread(file.data(), 1, file.size(), f) == file.size());
        ssd_png_info info;
        REQUIRE(parse_exact(file, &info) == code);
        if (stream_bytes >= 0) {
            const size_t pixels = (size_t)H * W * 3;
            unsigned char* stream = new unsigned char[(size_t)stream_bytes];
            unsigned char* want = new unsigned char[pixels];
            unsigned char* got = new unsigned char[pixels];
            REQUIRE(fread(stream, 1, (size_t)stream_bytes, f) == (size_t)stream_bytes);
            REQUIRE(fread(want, 1, pixels, f) == pixels);
            REQUIRE(info.height == H && info.width == W && info.stream_bytes == stream_bytes);
            REQUIRE(ssd_png_decode_host(&info, stream, (size_t)stream_bytes, got, pixels) == SSD_OK);
            REQUIRE(memcmp(got, want, pixels) == 0);
            REQUIRE(ssd_png_decode_host(&info, stream, (size_t)stream_bytes - 1, got, pixels) == SSD_E_INVALID);
            REQUIRE(ssd_png_decode_host(&info, stream, (size_t)stream_bytes, got, pixels - 1) == SSD_E_INVALID);
            delete[] stream;
            delete[] want;
            delete[] got;
            ++decoded;
        }
        if (n < 3) {
            for (size_t cut = 0; cut < file.size(); ++cut) {
                std::vector<unsigned char> part(file.begin(), file.begin() + (long)cut);
                REQUIRE(parse_exact(part, &info) != SSD_OK);
                ++mangled;
            }
            for (size_t at = 0; at < file.size(); ++at) {
                for (const int flip : {0x01, 0x80, 0xFF}) {
                    std::vector<unsigned char> bad(file);
                    bad[at] = (unsigned char)(bad[at] ^ flip);
                    still_accepted += parse_exact(bad, &info) == SSD_OK;
                    ++mangled;
                }
            }
        }
        ++n;
    }
    fclose(f);
    if (n == 0 || decoded == 0) { fprintf(stderr, "no cases\n"); return 1; }
    printf("png_decode_host_check: %d files parsed as expected, %d decoded to Pillow's pixels, %ld truncations and corruptions answered (%ld still accepted)\n",
           n, decoded, mangled, still_accepted);
    return 0;
}
