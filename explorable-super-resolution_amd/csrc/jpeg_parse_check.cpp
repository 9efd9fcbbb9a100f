// Stand-alone robustness check of the JPEG entropy decoder (esr_jpeg_parse.h), meant to be built with -fsanitize=address,undefined by
// tests/test_host_jpeg_file.py:  jpeg_parse_check FILE...
// For every file: the whole file must decode; every proper prefix must be refused; every single-byte substitution by 0x00, 0xFF and 0xD9
// must come back with ESR_OK, ESR_E_UNSUPPORTED or ESR_E_DATA.  Every input is handed over in a heap block of exactly its size, and the
// scan buffer is sized from the info call as the Python binding sizes it, so that a read or write past either end is the sanitizer's to see.
// Exit status 0: all of it held.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "esr_jpeg_parse.h"

static int decode_exact(const uint8_t* bytes, int64_t n) {
    uint8_t* copy = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);
    if (!copy) return 100;
    if (n > 0) memcpy(copy, bytes, (size_t)n);
    esr_jpeg::Info info;
    int rc = esr_jpeg::file_info(copy, n, &info);
    if (rc == esr_jpeg::OK) {
        int16_t* scan = (int16_t*)malloc((size_t)(64 * info.scan_blocks) * sizeof(int16_t) + 1);
        uint16_t tables[4 * 64];
        if (!scan) {
            free(copy);
            return 100;
        }
        rc = esr_jpeg::file_decode(copy, n, scan, 64 * info.scan_blocks, tables, &info);
        free(scan);
    }
    free(copy);
    return rc;
}

int main(int argc, char** argv) {
    long calls = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "%s: cannot open\n", argv[a]);
            return 1;
        }
        std::vector<uint8_t> file;
        uint8_t chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) file.insert(file.end(), chunk, chunk + got);
        fclose(f);
        const int64_t n = (int64_t)file.size();
        if (decode_exact(file.data(), n) != esr_jpeg::OK) {
            fprintf(stderr, "%s: the whole file does not decode\n", argv[a]);
            return 2;
        }
        for (int64_t k = 0; k < n; ++k, ++calls) {
            const int rc = decode_exact(file.data(), k);
            if (rc != esr_jpeg::E_DATA && rc != esr_jpeg::E_UNSUPPORTED) {
                fprintf(stderr, "%s: prefix of %lld bytes returned %d\n", argv[a], (long long)k, rc);
                return 3;
            }
        }
        const uint8_t values[3] = {0x00, 0xFF, 0xD9};
        for (int64_t k = 0; k < n; ++k) {
            const uint8_t kept = file[(size_t)k];
            for (int v = 0; v < 3; ++v, ++calls) {
                file[(size_t)k] = values[v];
                const int rc = decode_exact(file.data(), n);
                if (rc != esr_jpeg::OK && rc != esr_jpeg::E_DATA && rc != esr_jpeg::E_UNSUPPORTED) {
                    fprintf(stderr, "%s: byte %lld = 0x%02X returned %d\n", argv[a], (long long)k, values[v], rc);
                    return 4;
                }
            }
            file[(size_t)k] = kept;
        }
    }
    printf("%ld calls\n", calls);
    return 0;
}
