// Stand-alone check of the device inflater's host model under a sanitizer (CPU only; never loaded into Python, needs no
// GPU).  Links csrc/ssd_png_inflate.hip with an error sink of its own and reads the cases
// tests/micro/png_inflate_host_check.sh dumps from tests/png_inflate_cases.py: per case five int32 -- the stream's size, H,
// row_bytes, the status word ssd_png_inflate_host must give, 0 -- then the stream and, where the status is 0, zlib's bytes.
// Every buffer handed to the library is a heap block of exactly the size it is told, so a read or write outside it is an
// AddressSanitizer report.  Then every truncation and every single-byte corruption of the first three streams goes through:
// any status is fine, any report is not.  (Whether a corruption that is still accepted is one zlib accepts too, with the
// same bytes -- an Adler-32 can collide -- is tests/test_png_inflate_cpu.py's business: this program has no zlib.)
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

// the stream and the output as heap blocks of their own sizes: the status word, the bytes in `out`
static int inflate_exact(const std::vector<unsigned char>& stream, const size_t out_bytes, const long long rb, std::vector<unsigned char>* out) {
    unsigned char* in = new unsigned char[stream.size() ? stream.size() : 1];
    if (!stream.empty()) memcpy(in, stream.data(), stream.size());
    unsigned char* block = new unsigned char[out_bytes];
    memset(block, 0xA5, out_bytes);
    int status = -1;
    const int rc = ssd_png_inflate_host(in, stream.size(), block, out_bytes, rb, &status);
    if (out) out->assign(block, block + out_bytes);
    delete[] block;
    delete[] in;
    return rc == SSD_OK ? status : -2;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0, accepted = 0, refused = 0;
    long mangled = 0, still_accepted = 0;
    int head[5];
    while (fread(head, sizeof(int), 5, f) == 5) {
        const int stream_bytes = head[0], H = head[1], rb = head[2], status = head[3];
        const size_t out_bytes = (size_t)H * (size_t)(1 + rb);
        std::vector<unsigned char> stream((size_t)stream_bytes), want, got;
        REQUIRE(fread(stream.data(), 1, stream.size(), f) == stream.size());
        REQUIRE(inflate_exact(stream, out_bytes, rb, &got) == status);
        if (status == 0) {
            want.resize(out_bytes);
            REQUIRE(fread(want.data(), 1, out_bytes, f) == out_bytes);
            REQUIRE(got == want);
            ++accepted;
        } else {
            ++refused;
        }
        if (n < 3) {
            REQUIRE(status == 0);
            for (size_t cut = 0; cut < stream.size(); ++cut) {
                std::vector<unsigned char> part(stream.begin(), stream.begin() + (long)cut);
                REQUIRE(inflate_exact(part, out_bytes, rb, nullptr) > 0);
                ++mangled;
            }
            for (size_t at = 0; at < stream.size(); ++at) {
                for (const int flip : {0x01, 0x80, 0xFF}) {
                    std::vector<unsigned char> bad(stream);
                    bad[at] = (unsigned char)(bad[at] ^ flip);
                    const int st = inflate_exact(bad, out_bytes, rb, nullptr);
                    REQUIRE(st >= 0);
                    still_accepted += st == 0;
                    ++mangled;
                }
            }
        }
        ++n;
    }
    fclose(f);
    if (accepted == 0 || refused == 0) { fprintf(stderr, "no cases\n"); return 1; }
    printf("png_inflate_host_check: %d streams inflated to zlib's bytes, %d refused with the documented bit, %ld truncations and corruptions answered "
           "(%ld still accepted)\n", accepted, refused, mangled, still_accepted);
    return 0;
}
