// Entropy decoding of baseline JPEG files (ITU-T T.81) down to the quantised coefficients: the host side of esr_jpeg_file_info /
// esr_jpeg_file_decode (esr_jpeg_file.hip).  Plain C++ with no dependency on HIP or on the rest of the library, so that a stand-alone program
// can include it (jpeg_parse_check.cpp, built with sanitizers by tests/test_host_jpeg_file.py).
//
// Accepted: SOF0 and SOF1 (Huffman, 8-bit samples); one interleaved scan of 1 component, or of 3 components (YCbCr; a file that an Adobe
// APP14 segment marks as RGB is refused) at 4:2:0 or 4:4:4; 8- and 16-bit
// DQT entries; any number of DHT / DQT segments, tables redefined before the scan; APPn / COM of any length; fill 0xFF bytes before markers;
// 0xFF00 stuffing; DRI with RSTn (predictor reset, numbers cycling modulo 8); EOB, ZRL, categories up to 11 (DC) and 10 (AC).
// Everything else is refused with a code and a reason, never with a crash: every read is checked against the byte count, the marker loop
// advances by at least one byte per turn, and the block loop runs over a block count that the byte count bounds (a block takes at least
// two bits, so a header that announces more than 4 blocks per byte is refused as truncated before anything is decoded).
//
// Output (decode): the quantised coefficients as int16 in scan order — MCU after MCU, the blocks of an MCU in the order of T.81 A.2.3 (for
// 4:2:0 the 2 x 2 Y blocks row-major, then Cb, then Cr), 64 values per block in zigzag order, DC prediction undone — and the four
// quantisation tables in natural (row-major u, v) order as uint16 (0 where a table was never defined).
#pragma once
#include <stdint.h>
#include <string.h>

namespace esr_jpeg {

enum Status { OK = 0, E_ARG = -1, E_UNSUPPORTED = -2, E_DATA = -4 };      // ESR_OK, ESR_E_ARG, ESR_E_UNSUPPORTED, ESR_E_DATA

enum Reason {
    R_NONE = 0,
    // E_UNSUPPORTED
    R_PROGRESSIVE = 1, R_SOF_KIND = 2, R_ARITHMETIC = 3, R_PRECISION = 4, R_SCANS = 5, R_SAMPLING = 6, R_COMPONENTS = 7, R_COLORSPACE = 8,
    // E_DATA
    R_TRUNCATED = 32, R_BAD_CODE = 33, R_RUN = 34, R_NO_TABLE = 35, R_RST = 36, R_DIMENSION = 37, R_SEGMENT = 38, R_NOT_JPEG = 39
};

struct Info {                      // esr_jpeg_info (include/esr_hip.h): the same fields in the same order
    int32_t width, height, components, sof, restart_interval, mcus_h, mcus_w, blocks_per_mcu, reason, reserved;
    int32_t h[4], v[4], tq[4], blocks_h[4], blocks_w[4];
    int64_t scan_blocks;
};

static const uint8_t ZIGZAG[64] = {      // natural index (8u + v) of the k-th coefficient of the scan (T.81 figure A.6)
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined;
    int32_t mincode[17], maxcode[17], valptr[17];      // per code length 1..16; maxcode -1: no code of this length
    int32_t nvals;
    uint8_t vals[256];
    uint16_t fast[512];                                 // by the next 9 bits: (length << 8) | symbol, 0: longer than 9 bits or no code
};

struct Parser {
    const uint8_t* d;
    int64_t n, p;
    Info info;
    uint16_t qt[4][64];
    bool qt_defined[4];
    Huff huff[2][4];                                    // [class: 0 DC, 1 AC][id]
    int comp_id[4], td[4], ta[4];
    bool have_sof;
    int adobe_transform;      // of an Adobe APP14 segment; -1: none seen
    int status;

    int fail(int st, int reason) {
        status = st;
        info.reason = reason;
        return st;
    }
    int data(int reason) { return fail(E_DATA, reason); }
    bool have(int64_t k) const { return k >= 0 && p <= n - k; }
    int u8() { return d[p++]; }                          // callers check have() first
    int u16() {
        const int v = (d[p] << 8) | d[p + 1];
        p += 2;
        return v;
    }

    void init(const uint8_t* bytes, int64_t count) {
        d = bytes;
        n = count;
        p = 0;
        memset(&info, 0, sizeof(info));
        memset(qt, 0, sizeof(qt));
        memset(qt_defined, 0, sizeof(qt_defined));
        memset(huff, 0, sizeof(huff));
        have_sof = false;
        adobe_transform = -1;
        status = OK;
    }

    // the next marker's code: any bytes in front of it are skipped, as are fill 0xFF bytes; < 0 at the end of the data
    int next_marker() {
        while (p < n) {
            if (d[p++] != 0xFF) continue;
            while (p < n && d[p] == 0xFF) ++p;
            if (p >= n) return -1;
            const int m = d[p++];
            if (m != 0) return m;
        }
        return -1;
    }

    int read_dqt(int64_t end) {
        while (p < end) {
            const int pq_tq = u8(), pq = pq_tq >> 4, tq = pq_tq & 15;
            if (pq > 1 || tq > 3) return data(R_SEGMENT);
            if (end - p < 64 * (pq + 1)) return data(R_SEGMENT);
            for (int k = 0; k < 64; ++k) qt[tq][ZIGZAG[k]] = (uint16_t)(pq ? u16() : u8());
            qt_defined[tq] = true;
        }
        return OK;
    }

    int read_dht(int64_t end) {
        while (p < end) {
            if (end - p < 17) return data(R_SEGMENT);
            const int tc_th = u8(), tc = tc_th >> 4, th = tc_th & 15;
            if (tc > 1 || th > 3) return data(R_SEGMENT);
            int counts[17], total = 0;
            for (int l = 1; l <= 16; ++l) total += counts[l] = u8();
            if (total > 256 || end - p < total) return data(R_SEGMENT);
            Huff& h = huff[tc][th];
            memset(&h, 0, sizeof(h));
            h.nvals = total;
            for (int k = 0; k < total; ++k) h.vals[k] = (uint8_t)u8();
            int32_t code = 0, k = 0;
            for (int l = 1; l <= 16; ++l) {
                h.valptr[l] = k;
                h.mincode[l] = code;
                if ((int64_t)code + counts[l] > ((int64_t)1 << l)) return data(R_SEGMENT);      // more codes than the length holds
                for (int c = 0; c < counts[l]; ++c, ++code, ++k)
                    if (l <= 9)
                        for (int f = code << (9 - l); f < ((code + 1) << (9 - l)); ++f) h.fast[f] = (uint16_t)((l << 8) | h.vals[k]);
                h.maxcode[l] = counts[l] ? code - 1 : -1;
                code <<= 1;
            }
            h.defined = true;
        }
        return OK;
    }

    int read_sof(int marker, int64_t end) {
        if (have_sof) return data(R_SEGMENT);
        if (end - p < 6) return data(R_SEGMENT);
        const int precision = u8();
        info.sof = marker - 0xC0;
        info.height = u16();
        info.width = u16();
        info.components = u8();
        if (precision != 8) return fail(E_UNSUPPORTED, R_PRECISION);
        if (info.height == 0 || info.width == 0) return data(R_DIMENSION);
        if (info.components != 1 && info.components != 3)
            return info.components == 0 ? data(R_SEGMENT) : fail(E_UNSUPPORTED, R_COMPONENTS);
        if (end - p < 3 * info.components) return data(R_SEGMENT);
        for (int c = 0; c < info.components; ++c) {
            comp_id[c] = u8();
            const int hv = u8();
            info.h[c] = hv >> 4;
            info.v[c] = hv & 15;
            info.tq[c] = u8();
            if (info.h[c] < 1 || info.h[c] > 4 || info.v[c] < 1 || info.v[c] > 4 || info.tq[c] > 3) return data(R_SEGMENT);
        }
        int hmax = 1, vmax = 1;
        if (info.components == 1) {
            info.h[0] = info.v[0] = 1;                  // a one-component scan is not interleaved: its sampling factors say nothing (A.2.2)
        } else {
            const bool chroma11 = info.h[1] == 1 && info.v[1] == 1 && info.h[2] == 1 && info.v[2] == 1;
            const bool ok = chroma11 && ((info.h[0] == 2 && info.v[0] == 2) || (info.h[0] == 1 && info.v[0] == 1));
            if (!ok) return fail(E_UNSUPPORTED, R_SAMPLING);
            hmax = info.h[0];
            vmax = info.v[0];
        }
        info.mcus_w = (info.width + 8 * hmax - 1) / (8 * hmax);
        info.mcus_h = (info.height + 8 * vmax - 1) / (8 * vmax);
        info.blocks_per_mcu = 0;
        for (int c = 0; c < info.components; ++c) {
            info.blocks_w[c] = info.mcus_w * info.h[c];
            info.blocks_h[c] = info.mcus_h * info.v[c];
            info.blocks_per_mcu += info.h[c] * info.v[c];
        }
        info.scan_blocks = (int64_t)info.mcus_w * info.mcus_h * info.blocks_per_mcu;
        have_sof = true;
        return OK;
    }

    int read_sos(int64_t end) {
        if (!have_sof) return data(R_SEGMENT);
        if (end - p < 1) return data(R_SEGMENT);
        const int ns = u8();
        if (ns < 1 || ns > 4 || end - p != 2 * ns + 3) return data(R_SEGMENT);
        if (ns != info.components) return fail(E_UNSUPPORTED, R_SCANS);      // a scan of some of the components: others must follow
        for (int c = 0; c < ns; ++c) {
            const int id = u8(), t = u8();
            if (id != comp_id[c]) return data(R_SEGMENT);
            td[c] = t >> 4;
            ta[c] = t & 15;
            if (td[c] > 3 || ta[c] > 3) return data(R_SEGMENT);
        }
        const int ss = u8(), se = u8(), a = u8();
        if (ss != 0 || se != 63 || a != 0) return data(R_SEGMENT);
        for (int c = 0; c < ns; ++c)
            if (!huff[0][td[c]].defined || !huff[1][ta[c]].defined || !qt_defined[info.tq[c]]) return data(R_NO_TABLE);
        // three components are read as YCbCr (JFIF); Adobe's APP14 with transform 0 says they are RGB, which the models' mapping is not for
        if (info.components == 3 && adobe_transform == 0) return fail(E_UNSUPPORTED, R_COLORSPACE);
        // a block takes at least two bits (a DC code and an EOB code)
        if (info.scan_blocks > 4 * (n - p)) return data(R_TRUNCATED);
        return OK;
    }

    // Everything up to and including the SOS header: p is left at the first byte of the entropy-coded data.
    int read_headers() {
        if (!d || n < 0) return fail(E_ARG, R_NONE);
        if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) return data(n < 2 ? R_TRUNCATED : R_NOT_JPEG);
        p = 2;
        for (;;) {
            const int m = next_marker();
            if (m < 0) return data(R_TRUNCATED);
            if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // stand-alone markers with nothing to say here
            if (m == 0xD9) return data(R_TRUNCATED);                                // EOI before any scan
            if (!have(2)) return data(R_TRUNCATED);
            const int len = u16();
            if (len < 2) return data(R_SEGMENT);
            if (!have(len - 2)) return data(R_TRUNCATED);
            const int64_t end = p + len - 2;
            int rc = OK;
            if (m == 0xDB) rc = read_dqt(end);
            else if (m == 0xC4) rc = read_dht(end);
            else if (m == 0xC0 || m == 0xC1) rc = read_sof(m, end);
            else if (m == 0xC2) rc = fail(E_UNSUPPORTED, R_PROGRESSIVE);
            else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC8)) rc = fail(E_UNSUPPORTED, R_SOF_KIND);
            else if ((m >= 0xC9 && m <= 0xCF)) rc = fail(E_UNSUPPORTED, R_ARITHMETIC);          // SOF9-15 and DAC
            else if (m == 0xDD) {
                if (len != 4) return data(R_SEGMENT);
                info.restart_interval = u16();
            } else if (m == 0xEE) {
                if (len - 2 >= 12 && memcmp(d + p, "Adobe", 5) == 0) adobe_transform = d[p + 11];
            } else if (m == 0xDA) {
                rc = read_sos(end);
                if (rc != OK) return rc;
                p = end;
                return OK;
            }
            if (rc != OK) return rc;
            p = end;                                     // APPn, COM and whatever else carries a length: skipped
        }
    }

    // ---- the entropy-coded segment
    uint64_t acc;      // the low `cnt` bits are the next bits of the stream, the first of them on top
    int cnt;
    bool stop;         // a marker or the end of the data lies ahead: nothing more to take in

    void fill() {
        while (cnt <= 56 && !stop) {
            if (p >= n) { stop = true; break; }
            const uint8_t b = d[p];
            if (b == 0xFF) {
                if (p + 1 >= n || d[p + 1] != 0) { stop = true; break; }
                p += 2;                                  // 0xFF00: a stuffed 0xFF
            } else {
                ++p;
            }
            acc = (acc << 8) | b;
            cnt += 8;
        }
    }

    // s bits (0...16) as an unsigned number; < 0: the data ended
    int32_t receive(int s) {
        if (s == 0) return 0;
        if (cnt < s) {
            fill();
            if (cnt < s) return -1;
        }
        cnt -= s;
        return (int32_t)((acc >> cnt) & ((1u << s) - 1));
    }

    // the next Huffman symbol; < 0 with status set
    int decode(const Huff& h) {
        if (cnt < 16) fill();
        const uint32_t look = cnt >= 9 ? (uint32_t)((acc >> (cnt - 9)) & 511) : (uint32_t)((acc << (9 - cnt)) & 511);
        const uint16_t e = h.fast[look];
        if (e && (e >> 8) <= cnt) {
            cnt -= e >> 8;
            return e & 255;
        }
        int32_t code = 0;
        for (int l = 1; l <= 16; ++l) {
            if (cnt == 0) return data(R_TRUNCATED);
            --cnt;
            code = (code << 1) | (int32_t)((acc >> cnt) & 1);
            if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) {
                const int32_t k = h.valptr[l] + code - h.mincode[l];
                if (k >= h.nvals) return data(R_BAD_CODE);
                return h.vals[k];
            }
        }
        return data(R_BAD_CODE);
    }

    static int32_t extend(int32_t v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

    int decode_block(const Huff& dc, const Huff& ac, int32_t& pred, int16_t* out) {
        memset(out, 0, 64 * sizeof(int16_t));
        int s = decode(dc);
        if (s < 0) return status;
        if (s > 11) return data(R_BAD_CODE);
        if (s) {
            const int32_t v = receive(s);
            if (v < 0) return data(R_TRUNCATED);
            pred = (int16_t)(pred + extend(v, s));      // (kept inside int16 so that a corrupt file cannot overflow it)
        }
        out[0] = (int16_t)pred;
        for (int k = 1; k < 64;) {
            const int rs = decode(ac);
            if (rs < 0) return status;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
                if (r == 0) break;                       // EOB
                if (r != 15) return data(R_BAD_CODE);    // EOBn belongs to progressive scans
                k += 16;                                 // ZRL
                if (k > 64) return data(R_RUN);
                continue;
            }
            k += r;
            if (k > 63) return data(R_RUN);
            if (s > 10) return data(R_BAD_CODE);
            const int32_t v = receive(s);
            if (v < 0) return data(R_TRUNCATED);
            out[k++] = (int16_t)extend(v, s);
        }
        return OK;
    }

    // the scan (after read_headers) into scan[scan_blocks * 64], then the markers up to EOI
    int read_scan(int16_t* scan) {
        acc = 0;
        cnt = 0;
        stop = false;
        int32_t pred[4] = {0, 0, 0, 0};
        const int64_t mcus = (int64_t)info.mcus_w * info.mcus_h;
        const int ri = info.restart_interval;
        int expected_rst = 0;
        int16_t* out = scan;
        for (int64_t m = 0; m < mcus; ++m) {
            if (ri && m && m % ri == 0) {
                cnt = 0;                                 // the padding bits of the interval's last byte
                acc = 0;
                while (p < n && d[p] == 0xFF && p + 1 < n && d[p + 1] == 0xFF) ++p;      // fill bytes
                if (!have(2)) return data(R_TRUNCATED);
                if (d[p] != 0xFF || d[p + 1] != 0xD0 + expected_rst) return data(R_RST);
                p += 2;
                expected_rst = (expected_rst + 1) & 7;
                stop = false;
                pred[0] = pred[1] = pred[2] = pred[3] = 0;
            }
            for (int c = 0; c < info.components; ++c)
                for (int b = 0; b < info.h[c] * info.v[c]; ++b, out += 64)
                    if (decode_block(huff[0][td[c]], huff[1][ta[c]], pred[c], out) != OK) return status;
        }
        for (;;) {                                       // what follows the scan: EOI, or something this decoder does not take
            const int m = next_marker();
            if (m < 0) return data(R_TRUNCATED);
            if (m == 0xD9) return OK;
            if (m == 0xDA) return fail(E_UNSUPPORTED, R_SCANS);
            if (m >= 0xD0 && m <= 0xD7) return data(R_RST);
            if (m == 0xD8 || m == 0x01) continue;
            if (!have(2)) return data(R_TRUNCATED);
            const int len = u16();
            if (len < 2) return data(R_SEGMENT);
            if (!have(len - 2)) return data(R_TRUNCATED);
            p += len - 2;
        }
    }
};

// width, height, components, sampling and counts of a file; the status, with info->reason set also on failure
inline int file_info(const uint8_t* bytes, int64_t n, Info* info) {
    if (!bytes || !info || n < 0) return E_ARG;
    Parser ps;
    ps.init(bytes, n);
    const int rc = ps.read_headers();
    *info = ps.info;
    return rc;
}

// scan: scan_len int16 values, at least 64 per block of the file; tables: 4 x 64 uint16
inline int file_decode(const uint8_t* bytes, int64_t n, int16_t* scan, int64_t scan_len, uint16_t* tables, Info* info) {
    if (!bytes || !scan || !tables || n < 0) return E_ARG;
    Parser ps;
    ps.init(bytes, n);
    int rc = ps.read_headers();
    if (rc == OK && scan_len < 64 * ps.info.scan_blocks) rc = ps.fail(E_ARG, R_NONE);
    if (rc == OK) rc = ps.read_scan(scan);
    if (rc == OK) memcpy(tables, ps.qt, sizeof(ps.qt));
    if (info) *info = ps.info;
    return rc;
}

}  // namespace esr_jpeg
