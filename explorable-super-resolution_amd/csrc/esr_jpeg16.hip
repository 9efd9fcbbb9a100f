// The colour (4:2:0 chroma) half of the JPEG consistency layer (reference codes/JPEG_module/JPEG.py with chroma_mode, block size 16): the
// orthonormal 16x16 block DCT-II and its inverse between the planes of an image [B][C][H][W] and coefficient planes [B][Cc][H/16][W/16], where
// every image plane keeps K = 16 (channel 16u + v) or K = 8 (channel 8u + v, u, v < 8: the chroma down-sampling) frequencies per axis, with
// the per-image padded 16x16 tables, the rounding of the quantised chroma planes, and the chroma generator's sigmoid tail and its backward.
//
// Structure of esr_jpeg.hip: one workgroup owns 16 image rows x 16 blocks (256 pixels) of ONE plane, moves the image side as 16-byte accesses
// along W and the coefficient side as 16-byte accesses along w = W/16, and transposes through LDS in between:
//     image tile  X[16][16 blocks]  --row transform-->  T[r][v][j]  --column transform-->  O[K u + v][j]   (and the reverse for the inverse)
// X and O share one buffer.  LDS strides: a block of X takes 20 floats (its four 16-byte reads of 16 lanes fall on 16 different slots), a row
// of T 16 * 17 floats and a row of O 16, so the 4-byte accesses of a half-wave (two r or two v, sixteen j) walk 32 different banks.
//
// Cosines.  c(k, 15 - n) = (-1)^k c(k, n), so a 16-point transform is two 8-term sums over x[n] +- x[15 - n]: 128 cosines in place of 256 and
// half the multiply-adds (K * 8 per output vector).  The 128, computed in double on the host, are a by-value argument like the 8-point
// kernel's 64: the loops are unrolled, every cosine is a scalar operand, and the kernel-argument segment is read through the scalar cache in
// batches as the unrolled code walks the table — no LDS traffic and no vector register per cosine.  fp32 fmaf accumulation, no atomics: two
// calls give the same bits.
#include <math.h>

#include "esr_dct.h"

namespace {

constexpr int TB = 16;            // blocks per workgroup along W
constexpr int XB = 20;            // floats per block of an image row in LDS (16 + 4)
constexpr int XP = TB * XB;       // floats per image row of the tile
constexpr int TR = 16 * TB + 16;  // floats per r of T
constexpr int OP = TB;            // floats per coefficient row of O
constexpr int XO_FLOATS = 256 * OP > 16 * XP ? 256 * OP : 16 * XP;

// which planes a launch transforms, and where each lives in the tensors
struct Planes {
    int n;            // image planes transformed (grid z = B * n)
    int K[3];         // frequencies per axis: 8 or 16
    int tab[3];       // which of the image's three tables
    int rnd[3];       // rintf the result (forward only)
    float shift[3];   // subtracted from / added to the pixels
    int c_off[3];     // first channel of the plane in the coefficient tensor of c_C channels
    int y_off[3];     // first channel in y / dy / coef_out, tensors of y_C channels
    int img_C, c_C, y_C;
};

template <int K>
__device__ __forceinline__ void fwd_tile(const Dct16Tab& tab, float* XO, float* T, const float* qs, float shift, int divide, int do_round) {
    const int tid = threadIdx.x, hi = tid >> 4, j = tid & 15;
    {   // row transform: thread (r, j)
        float x[16], t[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a = *(const float4*)(XO + hi * XP + XB * j + 4 * q);
            x[4 * q] = a.x - shift; x[4 * q + 1] = a.y - shift; x[4 * q + 2] = a.z - shift; x[4 * q + 3] = a.w - shift;
        }
        dct16<K>(tab, x, t);
#pragma unroll
        for (int v = 0; v < K; ++v) T[hi * TR + v * TB + j] = t[v];
    }
    __syncthreads();
    if (hi < K) {   // column transform: thread (v, j)
        float t[16], c[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = T[r * TR + hi * TB + j];
        dct16<K>(tab, t, c);
#pragma unroll
        for (int u = 0; u < K; ++u) {
            const float q = qs[16 * u + hi];
            float s = divide ? c[u] / q : c[u] * q;
            if (do_round) s = rintf(s);
            XO[(u * K + hi) * OP + j] = s;
        }
    }
    __syncthreads();
}

template <int K>
__device__ __forceinline__ void inv_tile(const Dct16Tab& tab, float* XO, float* T, float shift) {
    const int tid = threadIdx.x, hi = tid >> 4, j = tid & 15;
    if (hi < K) {   // column transform: thread (v, j)
        float c[16], t[16];
#pragma unroll
        for (int u = 0; u < K; ++u) c[u] = XO[(u * K + hi) * OP + j];
        idct16<K>(tab, c, t);
#pragma unroll
        for (int r = 0; r < 16; ++r) T[r * TR + hi * TB + j] = t[r];
    }
    __syncthreads();
    {   // row transform: thread (r, j)
        float t[16], x[16];
#pragma unroll
        for (int v = 0; v < K; ++v) t[v] = T[hi * TR + v * TB + j];
        idct16<K>(tab, t, x);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(float4*)(XO + hi * XP + XB * j + 4 * q) = make_float4(x[4 * q] + shift, x[4 * q + 1] + shift, x[4 * q + 2] + shift, x[4 * q + 3] + shift);
    }
    __syncthreads();
}

// image -> coefficients, per plane:  c = DCT16(img - shift)[:K, :K] (/ or *) qtab, optionally rounded half to even
//   coef (optional): fp32 planes;  y / dy (optional, together): dy = c * s (1 - s), s = sigmoid(y)   (the chroma generator tail's backward)
__global__ __launch_bounds__(256) void dct16_fwd_kernel(const float* __restrict__ img, int h, int w, const float* __restrict__ qtab, Dct16Tab tab,
                                                        Planes pl, int divide, int vec, float* __restrict__ coef, const float* __restrict__ y,
                                                        float* __restrict__ dy) {
    __shared__ __attribute__((aligned(16))) float XO[XO_FLOATS];
    __shared__ float T[16 * TR];
    __shared__ float qs[256];
    const int tid = threadIdx.x, j0 = blockIdx.x * TB, i = blockIdx.y, b = blockIdx.z / pl.n, p = blockIdx.z % pl.n;
    const int nb = min(TB, w - j0);  // blocks of this tile inside the image
    const int K = pl.K[p];
    const long long W = 16ll * w;
    const float* src = img + (((long long)b * pl.img_C + p) * 16 * h + 16 * i) * W + 16 * j0;
    for (int k = tid; k < 16 * 4 * TB; k += 256) {
        const int r = k / (4 * TB), c4 = k % (4 * TB);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < 4 * nb) v = *(const float4*)(src + r * W + 4 * c4);
        *(float4*)(XO + r * XP + XB * (c4 >> 2) + 4 * (c4 & 3)) = v;
    }
    qs[tid] = qtab[((long long)b * 3 + pl.tab[p]) * 256 + tid];
    __syncthreads();
    if (K == 16) fwd_tile<16>(tab, XO, T, qs, pl.shift[p], divide, pl.rnd[p]);
    else fwd_tile<8>(tab, XO, T, qs, pl.shift[p], divide, pl.rnd[p]);
    for (int k = tid; k < K * K * (TB / 4); k += 256) {
        const int c = k / (TB / 4), jq = k % (TB / 4), jj = j0 + 4 * jq;
        if (jj >= w) continue;
        const long long o = (((long long)b * pl.c_C + pl.c_off[p] + c) * h + i) * w + jj;
        const long long oy = (((long long)b * pl.y_C + pl.y_off[p] + c) * h + i) * w + jj;
        coef_store4(*(const float4*)(XO + c * OP + 4 * jq), coef, y, dy, o, oy, vec, w - jj);
    }
}

// coefficients -> image, per plane:  c = coef [+ sigmoid(y) - 0.5];  img = shift + iDCT16(c (* or /) qtab, frequencies >= K zero);
// coef_out (optional) receives c
__global__ __launch_bounds__(256) void dct16_inv_kernel(const float* __restrict__ coef, const float* __restrict__ y, int h, int w,
                                                        const float* __restrict__ qtab, Dct16Tab tab, Planes pl, int divide, int vec,
                                                        float* __restrict__ coef_out, float* __restrict__ img) {
    __shared__ __attribute__((aligned(16))) float XO[XO_FLOATS];
    __shared__ float T[16 * TR];
    const int tid = threadIdx.x, j0 = blockIdx.x * TB, i = blockIdx.y, b = blockIdx.z / pl.n, p = blockIdx.z % pl.n;
    const int nb = min(TB, w - j0);
    const int K = pl.K[p];
    const float* qt = qtab + ((long long)b * 3 + pl.tab[p]) * 256;
    for (int k = tid; k < K * K * (TB / 4); k += 256) {
        const int c = k / (TB / 4), jq = k % (TB / 4), jj = j0 + 4 * jq;
        if (jj >= w) {   // beyond the row: blocks that are transformed and never stored
            *(float4*)(XO + c * OP + 4 * jq) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const long long o = (((long long)b * pl.c_C + pl.c_off[p] + c) * h + i) * w + jj;
        const long long oy = (((long long)b * pl.y_C + pl.y_off[p] + c) * h + i) * w + jj;
        *(float4*)(XO + c * OP + 4 * jq) = coef_load4(coef, y, coef_out, o, oy, vec, w - jj, qt + 16 * (c / K) + c % K, divide);
    }
    __syncthreads();
    if (K == 16) inv_tile<16>(tab, XO, T, pl.shift[p]);
    else inv_tile<8>(tab, XO, T, pl.shift[p]);
    const long long W = 16ll * w;
    float* dst = img + (((long long)b * pl.img_C + p) * 16 * h + 16 * i) * W + 16 * j0;
    for (int k = tid; k < 16 * 4 * TB; k += 256) {
        const int r = k / (4 * TB), c4 = k % (4 * TB);
        if (c4 < 4 * nb) *(float4*)(dst + r * W + 4 * c4) = *(const float4*)(XO + r * XP + XB * (c4 >> 2) + 4 * (c4 & 3));
    }
}

inline dim3 grid_of(int B, int n, int h, int w) { return dim3((unsigned)((w + TB - 1) / TB), (unsigned)h, (unsigned)(B * n)); }

// the compressor's three modes (ESR_JPEG16_*): planes Y, Cb, Cr of a three-plane image
Planes compress_planes(int mode) {
    Planes p = {};
    p.n = p.img_C = 3;
    const bool all = mode == ESR_JPEG16_ALL;
    for (int k = 0; k < 3; ++k) {
        p.K[k] = (k == 0 || all) ? 16 : 8;
        p.tab[k] = k;
        p.rnd[k] = (mode == ESR_JPEG16_QUANTIZE && k > 0) ? 1 : 0;
        p.shift[k] = k == 0 ? 128.f : 0.f;
        p.c_off[k] = all ? 256 * k : (k == 0 ? 0 : 256 + 64 * (k - 1));
    }
    p.c_C = all ? 768 : 384;
    return p;
}

// the extractor's three forms, by the coefficient tensor's channel count: 128 (Cb, Cr low), 512 (Cb, Cr full), 384 (Y full + Cb, Cr low)
bool extract_planes(int form, Planes* out) {
    Planes p = {};
    if (form != 128 && form != 384 && form != 512) return false;
    p.n = p.img_C = form == 384 ? 3 : 2;
    for (int k = 0; k < p.n; ++k) {
        const int ch = k + 3 - p.n;                    // 0 = Y, 1 = Cb, 2 = Cr
        p.K[k] = (ch == 0 || form == 512) ? 16 : 8;
        p.tab[k] = ch;
        p.shift[k] = ch == 0 ? 128.f : 0.f;
        p.c_off[k] = form == 384 ? (k == 0 ? 0 : 256 + 64 * (k - 1)) : p.K[k] * p.K[k] * k;
        p.y_off[k] = 64 * k;                           // (form 128 only)
    }
    p.c_C = form;
    p.y_C = 128;
    *out = p;
    return true;
}

}  // namespace

extern "C" int esr_jpeg16_compress(const float* x, int B, int H, int W, const float* qtab, int mode, float* coef, esr_stream_t stream) {
    if (!x || !qtab || !coef || B <= 0 || H <= 0 || W <= 0 || (H & 15) || (W & 15) || !al16(x) ||
        (mode != ESR_JPEG16_ALL && mode != ESR_JPEG16_DOWNSAMPLE && mode != ESR_JPEG16_QUANTIZE))
        return ESR_E_ARG;
    const int h = H / 16, w = W / 16;
    if (!grid_fits(B, 3, h)) return ESR_E_UNSUPPORTED;
    const Planes pl = compress_planes(mode);
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(dct16_fwd_kernel, grid_of(B, 3, h, w), dim3(256), 0, (hipStream_t)stream, x, h, w, qtab, dct16_tab(), pl, 1,
                       coef_vec(w, coef), coef, (const float*)nullptr, (float*)nullptr);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_jpeg16_extract(const float* coef, int coef_C, int coef_c0, const float* y, int form, int B, int h, int w, const float* qtab,
                                  float* coef_out, float* img, esr_stream_t stream) {
    Planes pl;
    if (!coef || !qtab || !img || !dims_positive(B, h, w) || !al16(img) || !extract_planes(form, &pl) || coef_c0 < 0 || coef_C < coef_c0 + form ||
        ((y || coef_out) && form != 128) || (coef_out && !y))
        return ESR_E_ARG;
    if (!grid_fits(B, pl.n, h)) return ESR_E_UNSUPPORTED;
    pl.c_C = coef_C;
    for (int k = 0; k < pl.n; ++k) pl.c_off[k] += coef_c0;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(dct16_inv_kernel, grid_of(B, pl.n, h, w), dim3(256), 0, (hipStream_t)stream, coef, y, h, w, qtab, dct16_tab(), pl, 0,
                       coef_vec(w, coef, y, coef_out), coef_out, img);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_jpeg16_extract_grad(const float* d_img, const float* y, int form, int B, int h, int w, const float* qtab, float* d_coef,
                                       float* d_y, esr_stream_t stream) {
    Planes pl;
    if (!d_img || !qtab || (!d_coef && !d_y) || (d_y && !y) || !dims_positive(B, h, w) || !al16(d_img) || !extract_planes(form, &pl) ||
        (d_y && form != 128))
        return ESR_E_ARG;
    if (!grid_fits(B, pl.n, h)) return ESR_E_UNSUPPORTED;
    for (int k = 0; k < pl.n; ++k) pl.shift[k] = 0.f;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(dct16_fwd_kernel, grid_of(B, pl.n, h, w), dim3(256), 0, (hipStream_t)stream, d_img, h, w, qtab, dct16_tab(), pl, 0,
                       coef_vec(w, d_coef, y, d_y), d_coef, d_y ? y : (const float*)nullptr, d_y);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_jpeg16_compress_grad(const float* d_coef, int mode, int B, int h, int w, const float* qtab, float* d_x, esr_stream_t stream) {
    if (!d_coef || !qtab || !d_x || !dims_positive(B, h, w) || !al16(d_x) ||
        (mode != ESR_JPEG16_ALL && mode != ESR_JPEG16_DOWNSAMPLE && mode != ESR_JPEG16_QUANTIZE))
        return ESR_E_ARG;
    if (!grid_fits(B, 3, h)) return ESR_E_UNSUPPORTED;
    Planes pl = compress_planes(mode);
    if (mode == ESR_JPEG16_QUANTIZE) pl.n = 1;         // the rounded chroma planes carry no gradient: the caller's d_x holds zeros there
    for (int k = 0; k < 3; ++k) pl.shift[k] = 0.f;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(dct16_inv_kernel, grid_of(B, pl.n, h, w), dim3(256), 0, (hipStream_t)stream, d_coef, (const float*)nullptr, h, w, qtab,
                       dct16_tab(), pl, 1, coef_vec(w, d_coef), (float*)nullptr, d_x);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
