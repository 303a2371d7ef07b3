// Stand-alone check of the device entropy decoder's host side under a sanitizer (CPU only; never loaded into Python, needs
// no GPU): ssd_jpeg_scan_plan and ssd_jpeg_entropy_decode_subseq, the host model that runs the kernels' decode core
// (csrc/ssd_jpeg_huff.h) through the kernels' phases.  Links csrc/ssd_jpeg.hip with an error sink of its own and reads the
// cases tests/micro/jpeg_unpack_host_check.sh dumps: per case the stream's size (int32), then struct ssd_jpeg_info of the
// SOUND stream it was made from, then the bytes -- the fixture, the real-size streams and the malformed set of
// tests/jpeg_unpack_cases.py.  Every buffer handed to the library is a heap block of exactly the size it is told, so a read
// or write outside it is an AddressSanitizer report.
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
    FILE* f = fopen(argc > 1 ? argv[1] : "jpeg_unpack_cases.bin", "rb");
    if (!f) { perror("cases"); return 2; }
    int n = 0, size = 0, sound = 0, refused = 0;
    while (fread(&size, sizeof(int), 1, f) == 1) {
        ssd_jpeg_info info;
        REQUIRE(fread(&info, sizeof(info), 1, f) == 1);
        std::vector<unsigned char> blob((size_t)size);                                 // exactly the stream: no byte after it
        REQUIRE(fread(blob.data(), 1, blob.size(), f) == blob.size());
        const size_t mcus = (size_t)info.mcus_x * info.mcus_y;
        const size_t nseg = info.restart_interval ? (mcus + info.restart_interval - 1) / info.restart_interval : 1;
        std::vector<short> want((size_t)info.coef_bytes / 2);
        const int host = ssd_jpeg_entropy_decode(blob.data(), blob.size(), &info, want.data(), want.size() * 2);
        REQUIRE(host == SSD_OK || host == SSD_E_INVALID);
        struct ssd_jpeg_scan_plan plan;
        std::vector<ssd_jpeg_segment> segs(nseg);
        const int planned = ssd_jpeg_scan_plan(blob.data(), blob.size(), &info, &plan, segs.data(), segs.size());
        REQUIRE(planned == SSD_OK || planned == SSD_E_INVALID);
        if (planned == SSD_OK) {
            REQUIRE(plan.segments == (int)nseg && plan.data_begin <= plan.data_end && (size_t)plan.data_end <= blob.size());
            for (size_t s = 0; s < nseg; ++s)
                REQUIRE(plan.data_begin + segs[s].first_byte + segs[s].bytes <= plan.data_end);
        } else {
            REQUIRE(host != SSD_OK);                                                   // the plan refuses nothing the decoder takes
        }
        if (nseg > 1) {
            std::vector<ssd_jpeg_segment> few(nseg - 1);                               // one segment short: refused, not overrun
            REQUIRE(ssd_jpeg_scan_plan(blob.data(), blob.size(), &info, &plan, few.data(), few.size()) != SSD_OK);
        }
        for (const int bits : {128, 160, 1024}) {
            std::vector<short> got(want.size());
            const int rc = ssd_jpeg_entropy_decode_subseq(blob.data(), blob.size(), &info, got.data(), got.size() * 2, bits);
            REQUIRE(rc == SSD_OK || rc == SSD_E_INVALID);
            if (rc == SSD_OK) REQUIRE(host == SSD_OK && memcmp(got.data(), want.data(), want.size() * 2) == 0);
            if (host != SSD_OK) REQUIRE(rc != SSD_OK);
            if (planned != SSD_OK) REQUIRE(rc != SSD_OK);
        }
        if (!want.empty()) {
            std::vector<short> small(want.size() - 64);                                // one block short: refused, not overrun
            REQUIRE(ssd_jpeg_entropy_decode_subseq(blob.data(), blob.size(), &info, small.data(), small.size() * 2, 128) == SSD_E_INVALID);
        }
        sound += host == SSD_OK;
        refused += host != SSD_OK;
        ++n;
    }
    fclose(f);
    printf("%d cases (%d the host decoder takes, %d it refuses): the subsequence model agrees, nothing outside the buffers\n", n, sound, refused);
    return n > 0 && sound > 0 && refused > 0 ? 0 : 3;
}
