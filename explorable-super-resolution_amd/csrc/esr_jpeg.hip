// The JPEG consistency layer of the explorable JPEG decoder (reference codes/JPEG_module/JPEG.py): orthonormal 8x8 block DCT-II and its
// inverse between a one-channel image [B][1][H][W] and its coefficient planes [B][64][H/8][W/8] (channel 8u + v), with the per-image
// quantisation table, the rounding of the quantising compressor, and the generator's sigmoid tail and its backward fused in.
//
// Both directions are HBM-bound (64 multiply-adds per element in separable form against 8 bytes moved).  Image rows are contiguous along W
// and coefficient planes along w = W/8, so one workgroup owns 8 image rows x 32 blocks (256 pixels): it moves the image side as 16-byte
// accesses along W and the coefficient side as 16-byte accesses along w, and transposes through LDS in between:
//     image tile  X[8][256]  --row transform-->  T[r][v][j]  --column transform-->  O[8u + v][j]   (and the reverse for the inverse)
// X and O share one buffer (X is dead when O is written and the other way round); rows are padded so that the 16-byte LDS accesses stay
// aligned and the 4-byte ones walk consecutive banks.  The 64 cosines are computed in double on the host, once, and reach the kernel as
// a by-value argument: with the loops unrolled every coefficient is a scalar-register operand.  fp32 accumulation, no atomics: two calls
// give the same bits.
#include <math.h>

#include "esr_dct.h"

namespace {

constexpr int TB = 32;          // blocks per workgroup along W
constexpr int XP = TB * 8 + 4;  // floats per image row of the tile in LDS
constexpr int TP = TB + 1;      // floats per (r, v) row of T
constexpr int OP = TB + 4;      // floats per coefficient row of O (a multiple of 4: 16-byte reads)
constexpr int XO_FLOATS = 64 * OP > 8 * XP ? 64 * OP : 8 * XP;

// image -> coefficients:  c = DCT(img - shift) (/ or *) qtab, optionally rounded half to even
//   coef (optional): fp32 planes;  act (optional): the same values in the conv kernels' activation layout, groups [0, 8) of the view
//   y / dy (optional, together): dy = c * s (1 - s), s = sigmoid(y)   (the generator tail's backward)
__global__ __launch_bounds__(256) void dct_fwd_kernel(const float* __restrict__ img, int h, int w, const float* __restrict__ qtab, DctTab tab,
                                                      float shift, int divide, int do_round, int vec, float* __restrict__ coef,
                                                      const float* __restrict__ y, float* __restrict__ dy, uint4* act_hi, uint4* act_lo,
                                                      long long act_bs, long long act_cs, int act_fmt) {
    __shared__ __attribute__((aligned(16))) float XO[XO_FLOATS];
    __shared__ float T[64 * TP];
    __shared__ float qs[64];
    const int tid = threadIdx.x, j0 = blockIdx.x * TB, i = blockIdx.y, b = blockIdx.z;
    const int nb = min(TB, w - j0);  // blocks of this tile inside the image
    const long long W = 8ll * w;
    const float* src = img + ((long long)b * 8 * h + 8 * i) * W + 8 * j0;
    for (int k = tid; k < 8 * 2 * TB; k += 256) {
        const int r = k / (2 * TB), c4 = k % (2 * TB);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < 2 * nb) v = *(const float4*)(src + r * W + 4 * c4);
        *(float4*)(XO + r * XP + 4 * c4) = v;
    }
    if (tid < 64) qs[tid] = qtab[b * 64 + tid];
    __syncthreads();
    const int hi5 = tid >> 5, j = tid & 31;
    {   // row transform: thread (r, j)
        const float4 a = *(const float4*)(XO + hi5 * XP + 8 * j), c = *(const float4*)(XO + hi5 * XP + 8 * j + 4);
        const float x[8] = {a.x - shift, a.y - shift, a.z - shift, a.w - shift, c.x - shift, c.y - shift, c.z - shift, c.w - shift};
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            float s = 0.f;
#pragma unroll
            for (int n = 0; n < 8; ++n) s = fmaf(tab.c[8 * v + n], x[n], s);
            T[(hi5 * 8 + v) * TP + j] = s;
        }
    }
    __syncthreads();
    {   // column transform: thread (v, j)
        float t[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) t[r] = T[(r * 8 + hi5) * TP + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) s = fmaf(tab.c[8 * u + r], t[r], s);
            const float q = qs[8 * u + hi5];
            s = divide ? s / q : s * q;
            if (do_round) s = rintf(s);
            XO[(u * 8 + hi5) * OP + j] = s;
        }
    }
    __syncthreads();
    if (coef || dy) {
        for (int k = tid; k < 64 * (TB / 4); k += 256) {
            const int c = k / (TB / 4), jq = k % (TB / 4), jj = j0 + 4 * jq;
            if (jj >= w) continue;
            const long long o = (((long long)b * 64 + c) * h + i) * w + jj;
            coef_store4(*(const float4*)(XO + c * OP + 4 * jq), coef, y, dy, o, o, vec, w - jj);
        }
    }
    if (act_hi && j < nb) {  // thread (u, j): the eight v of one pixel vector of group u
        float s[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) s[v] = XO[(hi5 * 8 + v) * OP + j];
        store8(act_hi, act_lo, act_off(act_bs, act_cs, w, b, hi5, i, j0 + j), s, act_fmt);
    }
}

// coefficients -> image:  c = coef [+ sigmoid(y) - 0.5];  img = shift + iDCT(c (* or /) qtab);  coef_out (optional) receives c
__global__ __launch_bounds__(256) void dct_inv_kernel(const float* __restrict__ coef, const float* __restrict__ y, int h, int w,
                                                      const float* __restrict__ qtab, DctTab tab, float shift, int divide, int vec,
                                                      float* __restrict__ coef_out, float* __restrict__ img) {
    __shared__ __attribute__((aligned(16))) float XO[XO_FLOATS];
    __shared__ float T[64 * TP];
    const int tid = threadIdx.x, j0 = blockIdx.x * TB, i = blockIdx.y, b = blockIdx.z;
    const int nb = min(TB, w - j0);
    for (int k = tid; k < 64 * (TB / 4); k += 256) {
        const int c = k / (TB / 4), jq = k % (TB / 4), jj = j0 + 4 * jq;
        if (jj >= w) {   // beyond the row: blocks that are transformed and never stored
            *(float4*)(XO + c * OP + 4 * jq) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const long long o = (((long long)b * 64 + c) * h + i) * w + jj;
        *(float4*)(XO + c * OP + 4 * jq) = coef_load4(coef, y, coef_out, o, o, vec, w - jj, qtab + b * 64 + c, divide);
    }
    __syncthreads();
    const int hi5 = tid >> 5, j = tid & 31;
    {   // column transform: thread (v, j)
        float o[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = XO[(u * 8 + hi5) * OP + j];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float s = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) s = fmaf(tab.c[8 * u + r], o[u], s);
            T[(r * 8 + hi5) * TP + j] = s;
        }
    }
    __syncthreads();
    {   // row transform: thread (r, j)
        float t[8], x[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) t[v] = T[(hi5 * 8 + v) * TP + j];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            float s = 0.f;
#pragma unroll
            for (int v = 0; v < 8; ++v) s = fmaf(tab.c[8 * v + n], t[v], s);
            x[n] = s + shift;
        }
        *(float4*)(XO + hi5 * XP + 8 * j) = make_float4(x[0], x[1], x[2], x[3]);
        *(float4*)(XO + hi5 * XP + 8 * j + 4) = make_float4(x[4], x[5], x[6], x[7]);
    }
    __syncthreads();
    const long long W = 8ll * w;
    float* dst = img + ((long long)b * 8 * h + 8 * i) * W + 8 * j0;
    for (int k = tid; k < 8 * 2 * TB; k += 256) {
        const int r = k / (2 * TB), c4 = k % (2 * TB);
        if (c4 < 2 * nb) *(float4*)(dst + r * W + 4 * c4) = *(const float4*)(XO + r * XP + 4 * c4);
    }
}

inline dim3 grid_of(int B, int h, int w) { return dim3((unsigned)((w + TB - 1) / TB), (unsigned)h, (unsigned)B); }

}  // namespace

extern "C" int esr_jpeg_compress(const float* x, int B, int H, int W, const float* qtab, int round, float* coef, const esr_act_view* act_out,
                                 esr_stream_t stream) {
    if (!x || !qtab || (!coef && !(act_out && act_out->hi)) || B <= 0 || H <= 0 || W <= 0 || (H & 7) || (W & 7) || !al16(x)) return ESR_E_ARG;
    const int h = H / 8, w = W / 8;
    const bool act = act_out && act_out->hi;
    if (act && (act_out->ncg < 8 || act_out->H != h || act_out->W != w || (act_out->fmt != ESR_FMT_BF16 && act_out->fmt != ESR_FMT_F16))) return ESR_E_ARG;
    if (!grid_fits(B, 1, h)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(dct_fwd_kernel, grid_of(B, h, w), dim3(256), 0, (hipStream_t)stream, x, h, w, qtab, dct_tab(), 128.f, 1, round ? 1 : 0,
                       coef_vec(w, coef), coef, (const float*)nullptr, (float*)nullptr, act ? (uint4*)act_out->hi : nullptr,
                       act ? (uint4*)act_out->lo : nullptr, act ? (long long)act_out->batch_stride : 0ll, act ? (long long)act_out->cg_stride : 0ll,
                       act ? act_out->fmt : 0);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_jpeg_extract(const float* coef, const float* y, int B, int h, int w, const float* qtab, float* coef_out, float* img,
                                esr_stream_t stream) {
    if (!coef || !qtab || !img || !dims_positive(B, h, w) || !al16(img)) return ESR_E_ARG;
    if (!grid_fits(B, 1, h)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(dct_inv_kernel, grid_of(B, h, w), dim3(256), 0, (hipStream_t)stream, coef, y, h, w, qtab, dct_tab(), 128.f, 0,
                       coef_vec(w, coef, y, coef_out), coef_out, img);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_jpeg_extract_grad(const float* d_img, const float* y, int B, int h, int w, const float* qtab, float* d_coef, float* d_y,
                                     esr_stream_t stream) {
    if (!d_img || !qtab || (!d_coef && !d_y) || (d_y && !y) || !dims_positive(B, h, w) || !al16(d_img)) return ESR_E_ARG;
    if (!grid_fits(B, 1, h)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(dct_fwd_kernel, grid_of(B, h, w), dim3(256), 0, (hipStream_t)stream, d_img, h, w, qtab, dct_tab(), 0.f, 0, 0,
                       coef_vec(w, d_coef, y, d_y), d_coef, d_y ? y : (const float*)nullptr, d_y, (uint4*)nullptr,
                       (uint4*)nullptr, 0ll, 0ll, 0);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_jpeg_compress_grad(const float* d_coef, int B, int h, int w, const float* qtab, float* d_x, esr_stream_t stream) {
    if (!d_coef || !qtab || !d_x || !dims_positive(B, h, w) || !al16(d_x)) return ESR_E_ARG;
    if (!grid_fits(B, 1, h)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(dct_inv_kernel, grid_of(B, h, w), dim3(256), 0, (hipStream_t)stream, d_coef, (const float*)nullptr, h, w, qtab, dct_tab(),
                       0.f, 1, coef_vec(w, d_coef), (float*)nullptr, d_x);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
