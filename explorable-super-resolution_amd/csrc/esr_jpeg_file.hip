// JPEG files into the explorable decoder's inputs.  Host side: esr_jpeg_file_info / esr_jpeg_file_decode around the baseline entropy decoder
// of esr_jpeg_parse.h (no device involved).  Device side: esr_jpeg_file_unpack, one launch per file that turns the uploaded scan-order int16
// buffer into the models' fp32 coefficient tensors (and, optionally, the Y generator's activation-layout input).
//
// The scan buffer holds MCU after MCU, each bpm = y_h y_v + n_chroma blocks of 64 int16 in zigzag order.  One workgroup owns TM = 32
// consecutive MCUs of one MCU row: it reads their bytes as they lie (consecutive 16-byte vectors) into LDS, a block per 33 words so that the
// block index walks consecutive banks, and then stores, per channel and block row, runs of consecutive blocks (consecutive addresses, 128 or
// 256 bytes per run of a full tile).  Pure data movement: int16 -> fp32 is exact, the DC offsets are one fp32 add, two calls give the same bits.
#include "esr_common.h"
#include "esr_jpeg_parse.h"

#include <stddef.h>

// esr_jpeg_info (the public header) and esr_jpeg::Info (the parser's) are one layout, and the codes one set of numbers
#define SAME_FIELD(f) (offsetof(esr_jpeg_info, f) == offsetof(esr_jpeg::Info, f) && sizeof(esr_jpeg_info::f) == sizeof(esr_jpeg::Info::f))
static_assert(sizeof(esr_jpeg_info) == sizeof(esr_jpeg::Info), "esr_jpeg_info");
static_assert(SAME_FIELD(width) && SAME_FIELD(height) && SAME_FIELD(components) && SAME_FIELD(sof) && SAME_FIELD(restart_interval) &&
              SAME_FIELD(mcus_h) && SAME_FIELD(mcus_w) && SAME_FIELD(blocks_per_mcu) && SAME_FIELD(reason) && SAME_FIELD(h) && SAME_FIELD(v) &&
              SAME_FIELD(tq) && SAME_FIELD(blocks_h) && SAME_FIELD(blocks_w) && SAME_FIELD(scan_blocks), "esr_jpeg_info fields");
#undef SAME_FIELD
static_assert(ESR_OK == esr_jpeg::OK && ESR_E_DATA == esr_jpeg::E_DATA && ESR_E_UNSUPPORTED == esr_jpeg::E_UNSUPPORTED &&
              ESR_E_ARG == esr_jpeg::E_ARG, "status codes");
static_assert(ESR_JPEG_R_PROGRESSIVE == esr_jpeg::R_PROGRESSIVE && ESR_JPEG_R_SOF_KIND == esr_jpeg::R_SOF_KIND &&
              ESR_JPEG_R_ARITHMETIC == esr_jpeg::R_ARITHMETIC && ESR_JPEG_R_PRECISION == esr_jpeg::R_PRECISION &&
              ESR_JPEG_R_SCANS == esr_jpeg::R_SCANS && ESR_JPEG_R_SAMPLING == esr_jpeg::R_SAMPLING &&
              ESR_JPEG_R_COMPONENTS == esr_jpeg::R_COMPONENTS && ESR_JPEG_R_COLORSPACE == esr_jpeg::R_COLORSPACE &&
              ESR_JPEG_R_TRUNCATED == esr_jpeg::R_TRUNCATED && ESR_JPEG_R_BAD_CODE == esr_jpeg::R_BAD_CODE && ESR_JPEG_R_RUN == esr_jpeg::R_RUN &&
              ESR_JPEG_R_NO_TABLE == esr_jpeg::R_NO_TABLE && ESR_JPEG_R_RST == esr_jpeg::R_RST && ESR_JPEG_R_DIMENSION == esr_jpeg::R_DIMENSION &&
              ESR_JPEG_R_SEGMENT == esr_jpeg::R_SEGMENT && ESR_JPEG_R_NOT_JPEG == esr_jpeg::R_NOT_JPEG, "reason codes");

extern "C" int esr_jpeg_file_info(const uint8_t* bytes, int64_t n, esr_jpeg_info* info) {
    return esr_jpeg::file_info(bytes, n, reinterpret_cast<esr_jpeg::Info*>(info));
}

extern "C" int esr_jpeg_file_decode(const uint8_t* bytes, int64_t n, int16_t* scan, int64_t scan_len, uint16_t* tables, esr_jpeg_info* info) {
    return esr_jpeg::file_decode(bytes, n, scan, scan_len, tables, reinterpret_cast<esr_jpeg::Info*>(info));
}

namespace {

constexpr int TM = 32;          // MCUs per workgroup
constexpr int BW = 33;          // 32-bit words per block in LDS (64 int16 + one word of padding)
constexpr int MAX_BPM = 6;

struct ZigzagPos {
    unsigned char p[64];        // scan position of natural index 8u + v
};

const ZigzagPos& zigzag_pos() {
    static const ZigzagPos z = [] {
        ZigzagPos t;
        for (int k = 0; k < 64; ++k) t.p[esr_jpeg::ZIGZAG[k]] = (unsigned char)k;
        return t;
    }();
    return z;
}

__device__ __forceinline__ float lds_coef(const uint32_t* L, int block, int pos) {
    const uint32_t word = L[block * BW + (pos >> 1)];
    return (float)(short)((pos & 1) ? (word >> 16) : (word & 0xFFFFu));
}

__global__ __launch_bounds__(256) void unpack_kernel(const uint4* __restrict__ scan, int mcus_w, int y_h, int y_v, int n_chroma, float y_dc,
                                                     float c_dc, ZigzagPos zz, float* __restrict__ y_out, float* __restrict__ c_out, uint4* act_hi,
                                                     uint4* act_lo, long long act_cs, int act_fmt) {
    __shared__ uint32_t L[TM * MAX_BPM * BW];
    const int tid = threadIdx.x, m0 = blockIdx.x * TM, mi = blockIdx.y;
    const int nm = min(TM, mcus_w - m0);                // MCUs of this tile inside the row
    const int ny = y_h * y_v, bpm = ny + n_chroma;
    const int mcus_h = gridDim.y;
    // the tile's bytes: nm * bpm blocks of 8 vectors, consecutive in the scan buffer
    const uint4* src = scan + ((long long)mi * mcus_w + m0) * bpm * 8;
    for (int k = tid; k < nm * bpm * 8; k += 256) {
        const uint4 v = src[k];
        uint32_t* dst = L + (k >> 3) * BW + (k & 7) * 4;
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    __syncthreads();
    const int wj = TM * y_h;                            // blocks of a full tile along a block row
    const int H8 = mcus_h * y_v, W8 = mcus_w * y_h;
    if (y_out) {
        for (int k = tid; k < y_v * 64 * wj; k += 256) {
            const int jj = k % wj, c = (k / wj) & 63, r = k / (wj * 64);
            if (jj >= nm * y_h) continue;
            const int block = (jj / y_h) * bpm + r * y_h + jj % y_h;
            const float v = lds_coef(L, block, zz.p[c]) + (c == 0 ? y_dc : 0.f);
            y_out[((long long)c * H8 + (mi * y_v + r)) * W8 + (long long)m0 * y_h + jj] = v;
        }
    }
    if (c_out) {
        for (int k = tid; k < 128 * TM; k += 256) {
            const int j = k % TM, c = k / TM;           // c = 64 plane + 8u + v
            if (j >= nm) continue;
            const float v = lds_coef(L, j * bpm + ny + (c >> 6), zz.p[c & 63]) + ((c & 63) == 0 ? c_dc : 0.f);
            c_out[((long long)c * mcus_h + mi) * mcus_w + m0 + j] = v;
        }
    }
    if (act_hi) {                                       // the eight v of one pixel vector of group u
        for (int k = tid; k < y_v * 8 * wj; k += 256) {
            const int jj = k % wj, u = (k / wj) & 7, r = k / (wj * 8);
            if (jj >= nm * y_h) continue;
            const int block = (jj / y_h) * bpm + r * y_h + jj % y_h;
            float s[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) s[v] = lds_coef(L, block, zz.p[8 * u + v]);
            if (u == 0) s[0] += y_dc;
            store8(act_hi, act_lo, act_off(0ll, act_cs, W8, 0, u, mi * y_v + r, m0 * y_h + jj), s, act_fmt);
        }
    }
}

}  // namespace

extern "C" int esr_jpeg_file_unpack(const int16_t* scan, int mcus_h, int mcus_w, int y_h, int y_v, int n_chroma, float y_dc, float c_dc,
                                    float* y_out, float* c_out, const esr_act_view* act_out, esr_stream_t stream) {
    const bool act = act_out && act_out->hi;
    if (!scan || (!y_out && !c_out && !act) || mcus_h <= 0 || mcus_w <= 0 || !((y_h == 1 && y_v == 1) || (y_h == 2 && y_v == 2)) ||
        (n_chroma != 0 && n_chroma != 2) || (c_out && n_chroma != 2) || ((uintptr_t)scan & 15))
        return ESR_E_ARG;
    if (mcus_w > (1 << 28) || mcus_h > (1 << 28)) return ESR_E_ARG;
    if (act && (act_out->ncg < 8 || act_out->H != mcus_h * y_v || act_out->W != mcus_w * y_h ||
                (act_out->fmt != ESR_FMT_BF16 && act_out->fmt != ESR_FMT_F16)))
        return ESR_E_ARG;
    if (mcus_h > 65535) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((mcus_w + TM - 1) / TM), (unsigned)mcus_h), dim3(256), 0, (hipStream_t)stream,
                       (const uint4*)scan, mcus_w, y_h, y_v, n_chroma, y_dc, c_dc, zigzag_pos(), y_out, c_out, act ? (uint4*)act_out->hi : nullptr,
                       act ? (uint4*)act_out->lo : nullptr, act ? (long long)act_out->cg_stride : 0ll, act ? act_out->fmt : 0);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
