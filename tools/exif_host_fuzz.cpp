// exif_host_fuzz.cpp -- the EXIF orientation reader of the scanner (host/pjd_scan.cpp, pjd_scanned_orientation) under the sanitizers:
// every file given (tests/golden/exif/*.jpg) is scanned as it is, cut off at every length of its head, and with every byte of its
// head replaced by a few values -- length fields, offsets, counts and the byte-order mark among them.  Every copy lives in a heap
// block of exactly its size, so a read past the segment that leaves the file is a report; the result must be 1..8 whatever comes in.
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tools/exif_host_fuzz.cpp pim-jpeg-decoder_amd/host/pjd_scan.cpp -o exif_host_fuzz
//     ./exif_host_fuzz tests/golden/exif/*.jpg
//
// Deterministic and bounded: HEAD bytes of each file, a fixed set of replacement values.  Prints "no sanitizer report" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pjd_host.h"

static unsigned long g_scans = 0, g_hist[9] = {0};

static int scan(const uint8_t *data, size_t n)
{
    uint8_t *copy = (uint8_t *)malloc(n ? n : 1);            // exactly n bytes: the sanitizer sees the end of the file
    memcpy(copy, data, n);
    pjd_scanned *s = nullptr;
    pjd_scan_memory(copy, n, "f.jpg", &s);
    const int o = pjd_scanned_orientation(s);
    pjd_scanned_free(s);
    free(copy);
    g_scans++;
    if (o < 1 || o > 8) { printf("orientation %d is outside 1..8\n", o); exit(1); }
    g_hist[o]++;
    return o;
}

int main(int argc, char **argv)
{
    const size_t HEAD = 160;                                  // SOI and the inserted segments of every fixture lie in here
    static const uint8_t values[] = {0x00, 0x01, 0x7f, 0xff, 0xe1, 0x12};
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { printf("cannot open %s\n", argv[a]); return 1; }
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + k);
        fclose(f);
        scan(d.data(), d.size());
        const size_t head = d.size() < HEAD ? d.size() : HEAD;
        for (size_t n = 0; n <= head; n++) scan(d.data(), n);                        // cut off at every length
        for (size_t i = 0; i < head; i++) {
            const uint8_t keep = d[i];
            for (uint8_t v : values) { d[i] = v; scan(d.data(), d.size()); }
            d[i] = (uint8_t)(keep ^ 0x80); scan(d.data(), d.size());
            d[i] = keep;
        }
    }
    printf("%lu scans, orientations 1..8:", g_scans);
    for (int o = 1; o <= 8; o++) printf(" %lu", g_hist[o]);
    printf("\nno sanitizer report\n");
    return 0;
}
