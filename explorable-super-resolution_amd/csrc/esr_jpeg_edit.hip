// The editing tools of the explorable JPEG decoder (reference codes/GUI.py imprinting, codes/models/DecompCNN_model.py:316-334,
// codes/utils/util.py:328-330): the colour model's YCbCr -> RGB conversion and its adjoint, the score of a batch of candidate imprints (how far
// each leaves the set of images consistent with the compressed code), and the projection of a desired plane onto that set, 8- and 16-point.
// All four are HBM-bound; every value is read once and written once, in 16-byte accesses where the addresses allow.
//
// esr_ycbcr_rgb / _grad: a thread owns four consecutive pixels of one image and moves their three planes.
//
// The 8-point kernels (esr_jpeg_violation, esr_jpeg_pair).  The coefficient planes [64][h][w] of one image are contiguous over the h w blocks,
// so a workgroup owns E8_TB = 32 CONSECUTIVE blocks t = i w + j of one image (a tile may run over several block rows: a 64 x 64 candidate is two
// full tiles, where a tile of 32 blocks along W would be three quarters empty).  It stages the 8 x 8 pixels of its blocks (two 16-byte loads per
// block row: W is a multiple of 8 and the image 16-byte aligned) and its 64 x 32 coefficients (16-byte loads along t when h w is a multiple of 4
// and the pointer aligned, element by element otherwise) in LDS, runs the row transform into T[r][v][j] and the column transform in thread
// (v, j), which then holds the 8 coefficients (u, v) of block j in registers:
//   violation: it adds max(0, |c / q - coef| - 0.5) of its 8 coefficients (fp32 terms, fp64 sum, u ascending), the workgroup adds its threads in
//     a fixed order and writes ONE partial; a second launch adds the partials of a candidate.  The [N][64][h][w] tensor is never written.
//   pair: it clamps c / q to coef +- 0.5, multiplies by q and runs the inverse column transform on the same registers, back into the entries
//     of T it read (no other thread touches them); the inverse row transform and the image store follow.
// Which form staged the coefficients does not change the arithmetic or its order: the 16-byte and the scalar path give the same bits.
//
// The 16-point kernel (esr_jpeg16_pair) has the tile of esr_jpeg16.hip (16 image rows x 16 blocks of one chroma plane) and the same flow with
// K = 16: all 256 frequencies are divided by the padded table and multiplied back (as the reference's 512-channel extractor form does), and only
// u, v < 8 are clamped, against the 64 quantised coefficients of the plane.
// No atomics anywhere: two calls give the same bits.
#include "esr_dct.h"

namespace {

constexpr int ED_THREADS = 256;
constexpr int ED_WAVES = ED_THREADS / 64;

// ------------------------------------------------------------------------------------------------ YCbCr <-> RGB
struct Affine3 {
    float m[9];    // out[r] = sum_c m[3 r + c] (in[c] / pre) + off[r], then / post
    float off[3];
    float pre, post;
};

// (every operation spelled out, so that the 16-byte and the element-by-element path round alike whatever the compiler would contract)
__device__ __forceinline__ void affine3(const Affine3& a, const float (&x)[3], float (&o)[3]) {
    const float t0 = __fdiv_rn(x[0], a.pre), t1 = __fdiv_rn(x[1], a.pre), t2 = __fdiv_rn(x[2], a.pre);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float s = fmaf(a.m[3 * r + 2], t2, fmaf(a.m[3 * r + 1], t1, __fmul_rn(a.m[3 * r], t0)));
        o[r] = __fdiv_rn(__fadd_rn(s, a.off[r]), a.post);
    }
}

// x, out: [B][3][n]; a thread owns pixels 4 i .. 4 i + 3 of image blockIdx.y
__global__ __launch_bounds__(ED_THREADS) void affine3_kernel(const float* __restrict__ x, long long n, Affine3 a, int vec, float* __restrict__ out) {
    const long long i = 4 * ((long long)blockIdx.x * ED_THREADS + threadIdx.x);
    if (i >= n) return;
    const long long base = (long long)blockIdx.y * 3 * n + i;
    if (vec) {
        const float4 p0 = *(const float4*)(x + base), p1 = *(const float4*)(x + base + n), p2 = *(const float4*)(x + base + 2 * n);
        const float e0[4] = {p0.x, p0.y, p0.z, p0.w}, e1[4] = {p1.x, p1.y, p1.z, p1.w}, e2[4] = {p2.x, p2.y, p2.z, p2.w};
        float r[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float in[3] = {e0[k], e1[k], e2[k]};
            float o[3];
            affine3(a, in, o);
            r[0][k] = o[0]; r[1][k] = o[1]; r[2][k] = o[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *(float4*)(out + base + c * n) = make_float4(r[c][0], r[c][1], r[c][2], r[c][3]);
    } else {
        for (int k = 0; k < 4 && i + k < n; ++k) {
            const float in[3] = {x[base + k], x[base + n + k], x[base + 2 * n + k]};
            float o[3];
            affine3(a, in, o);
            out[base + k] = o[0]; out[base + n + k] = o[1]; out[base + 2 * n + k] = o[2];
        }
    }
}

// the reference's matrix (utils/util.py:329; models/DecompCNN_model.py:36-38 here): mat[r][c] = (float)(255 M[c][r]), offset[r] = (float)o[r] / 255
Affine3 ycbcr_rgb_map(bool adjoint) {
    static const double M[3][3] = {{0.00456621, 0.00456621, 0.00456621}, {0, -0.00153632, 0.00791071}, {0.00625893, -0.00318811, 0}};
    static const float O[3] = {-222.921f, 135.576f, -276.836f};
    Affine3 a;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const float v = (float)(255.0 * M[c][r]);
            a.m[adjoint ? 3 * c + r : 3 * r + c] = v;
        }
    for (int r = 0; r < 3; ++r) a.off[r] = adjoint ? 0.f : O[r] / 255.f;
    a.pre = adjoint ? 1.f : 255.f;
    a.post = adjoint ? 255.f : 1.f;
    return a;
}

int launch_affine3(const float* x, int B, int H, int W, bool adjoint, float* out, esr_stream_t stream) {
    if (!x || !out || B <= 0 || H <= 0 || W <= 0) return ESR_E_ARG;
    const long long n = (long long)H * W, blocks = (n + 4 * ED_THREADS - 1) / (4 * ED_THREADS);
    if (B > 65535 || blocks > 0x7FFFFFFFll) return ESR_E_UNSUPPORTED;
    const int vec = (n % 4 == 0 && al16(x) && al16(out)) ? 1 : 0;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(affine3_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(ED_THREADS), 0, (hipStream_t)stream, x, n, ycbcr_rgb_map(adjoint), vec, out);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

// ------------------------------------------------------------------------------------------------ reductions
// sum of v over the workgroup, in thread 0, in a fixed order: lanes by shuffles, then the waves one after the other
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < ED_WAVES; ++w) v += red[w];
    return v;
}

// out[b] = sum_i partial[b][i], i < n: thread t adds i = t, t + 256, ... in order, then block_sum
__global__ __launch_bounds__(ED_THREADS) void sum_partials_kernel(const double* __restrict__ partial, long long n, double* __restrict__ out) {
    __shared__ double red[ED_WAVES];
    const double* p = partial + (long long)blockIdx.x * n;
    double v = 0.0;
    for (long long i = threadIdx.x; i < n; i += ED_THREADS) v += p[i];
    v = block_sum(v, red);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// ------------------------------------------------------------------------------------------------ 8-point tiles
constexpr int E8_TB = 32;             // blocks per workgroup, consecutive in t = i w + j
constexpr int E8_XP = E8_TB * 8 + 4;  // floats per image row of the tile in LDS
constexpr int E8_TP = E8_TB + 1;      // floats per (r, v) row of T
constexpr int E8_OP = E8_TB + 4;      // floats per coefficient row (a multiple of 4: 16-byte stores)

struct Tile8 {
    int t0, nb;        // first block of the tile and how many of its E8_TB lie inside the image
    long long img;     // element offset of the image plane
};

__device__ __forceinline__ Tile8 tile8(long long image, int tile, int h, int w) {
    Tile8 t;
    t.t0 = tile * E8_TB;
    t.nb = min(E8_TB, h * w - t.t0);
    t.img = image * 64 * h * w;
    return t;
}

// X[r][8 j + s] = img[8 i + r][8 jj + s] of block t0 + j = (i, jj); zeros beyond the image
__device__ __forceinline__ void load_image8(const float* __restrict__ img, const Tile8& t, int w, float* X) {
    const long long W = 8ll * w;
    for (int k = threadIdx.x; k < 8 * 2 * E8_TB; k += ED_THREADS) {
        const int r = k / (2 * E8_TB), c4 = k % (2 * E8_TB), j = c4 >> 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < t.nb) {
            const int blk = t.t0 + j, i = blk / w, jj = blk % w;
            v = *(const float4*)(img + t.img + (8ll * i + r) * W + 8 * jj + 4 * (c4 & 1));
        }
        *(float4*)(X + r * E8_XP + 4 * c4) = v;
    }
}

__device__ __forceinline__ void store_image8(float* __restrict__ img, const Tile8& t, int w, const float* X) {
    const long long W = 8ll * w;
    for (int k = threadIdx.x; k < 8 * 2 * E8_TB; k += ED_THREADS) {
        const int r = k / (2 * E8_TB), c4 = k % (2 * E8_TB), j = c4 >> 1;
        if (j >= t.nb) continue;
        const int blk = t.t0 + j, i = blk / w, jj = blk % w;
        *(float4*)(img + t.img + (8ll * i + r) * W + 8 * jj + 4 * (c4 & 1)) = *(const float4*)(X + r * E8_XP + 4 * c4);
    }
}

// Q[c][j] = coef[c][t0 + j] of one image's planes (`coef` points at them); zeros beyond the image
__device__ __forceinline__ void load_coef8(const float* __restrict__ coef, const Tile8& t, int hw, int vec, float* Q) {
    for (int k = threadIdx.x; k < 64 * (E8_TB / 4); k += ED_THREADS) {
        const int c = k / (E8_TB / 4), jq = k % (E8_TB / 4), n = t.nb - 4 * jq;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        if (n > 0) {
            const float* p = coef + (long long)c * hw + t.t0 + 4 * jq;
            if (vec) {
                const float4 v = *(const float4*)p;
                e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
            } else {
                for (int m = 0; m < 4 && m < n; ++m) e[m] = p[m];
            }
        }
        *(float4*)(Q + c * E8_OP + 4 * jq) = make_float4(e[0], e[1], e[2], e[3]);
    }
}

// X -> T[r][v][j] (thread (r, j)), then thread (v, j) gets o[u] = DCT(X - 128)[u][v] / q[u][v] of block j.  Ends without a barrier: the thread
// has read exactly the entries T[.][v][j], which it alone may write next.
__device__ __forceinline__ void forward8(const DctTab& tab, const float* X, float* T, const float* qs, float shift, float (&o)[8]) {
    const int hi5 = threadIdx.x >> 5, j = threadIdx.x & 31;
    {
        const float4 a = *(const float4*)(X + hi5 * E8_XP + 8 * j), c = *(const float4*)(X + hi5 * E8_XP + 8 * j + 4);
        const float x[8] = {a.x - shift, a.y - shift, a.z - shift, a.w - shift, c.x - shift, c.y - shift, c.z - shift, c.w - shift};
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            float s = 0.f;
#pragma unroll
            for (int n = 0; n < 8; ++n) s = fmaf(tab.c[8 * v + n], x[n], s);
            T[(hi5 * 8 + v) * E8_TP + j] = s;
        }
    }
    __syncthreads();
    float t[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) t[r] = T[(r * 8 + hi5) * E8_TP + j];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) s = fmaf(tab.c[8 * u + r], t[r], s);
        o[u] = s / qs[8 * u + hi5];
    }
}

// thread (v, j) with its o[u] (already multiplied by q) -> T -> X[r][8 j + s] + shift
__device__ __forceinline__ void inverse8(const DctTab& tab, const float (&o)[8], float* T, float* X, float shift) {
    const int hi5 = threadIdx.x >> 5, j = threadIdx.x & 31;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) s = fmaf(tab.c[8 * u + r], o[u], s);
        T[(r * 8 + hi5) * E8_TP + j] = s;
    }
    __syncthreads();
    float t[8], x[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) t[v] = T[(hi5 * 8 + v) * E8_TP + j];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) s = fmaf(tab.c[8 * v + n], t[v], s);
        x[n] = s + shift;
    }
    *(float4*)(X + hi5 * E8_XP + 8 * j) = make_float4(x[0], x[1], x[2], x[3]);
    *(float4*)(X + hi5 * E8_XP + 8 * j + 4) = make_float4(x[4], x[5], x[6], x[7]);
    __syncthreads();
}

// grid x = candidate * tiles + tile.  coef_bs / q_bs: elements between two candidates' coefficients / tables (0: one for all)
__global__ __launch_bounds__(ED_THREADS) void violation_kernel(const float* __restrict__ cand, int h, int w, int tiles, const float* __restrict__ coef,
                                                               long long coef_bs, const float* __restrict__ qtab, int q_bs, DctTab tab, int vec,
                                                               double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float X[8 * E8_XP];
    __shared__ __attribute__((aligned(16))) float Q[64 * E8_OP];
    __shared__ float T[64 * E8_TP];
    __shared__ float qs[64];
    __shared__ double red[ED_WAVES];
    const long long image = blockIdx.x / tiles;
    const Tile8 t = tile8(image, (int)(blockIdx.x % tiles), h, w);
    load_image8(cand, t, w, X);
    load_coef8(coef + image * coef_bs, t, h * w, vec, Q);
    if (threadIdx.x < 64) qs[threadIdx.x] = qtab[image * q_bs + threadIdx.x];
    __syncthreads();
    float o[8];
    forward8(tab, X, T, qs, 128.f, o);
    const int hi5 = threadIdx.x >> 5, j = threadIdx.x & 31;
    double acc = 0.0;
    if (j < t.nb) {
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)fmaxf(fabsf(o[u] - Q[(8 * u + hi5) * E8_OP + j]) - 0.5f, 0.f);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(ED_THREADS) void pair8_kernel(const float* __restrict__ desired, int h, int w, int tiles, const float* __restrict__ coef,
                                                           const float* __restrict__ qtab, DctTab tab, int vec, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float X[8 * E8_XP];
    __shared__ __attribute__((aligned(16))) float Q[64 * E8_OP];
    __shared__ float T[64 * E8_TP];
    __shared__ float qs[64];
    const long long image = blockIdx.x / tiles;
    const Tile8 t = tile8(image, (int)(blockIdx.x % tiles), h, w);
    load_image8(desired, t, w, X);
    load_coef8(coef + image * 64 * h * w, t, h * w, vec, Q);
    if (threadIdx.x < 64) qs[threadIdx.x] = qtab[image * 64 + threadIdx.x];
    __syncthreads();
    float o[8];
    forward8(tab, X, T, qs, 128.f, o);
    const int hi5 = threadIdx.x >> 5, j = threadIdx.x & 31;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float c = Q[(8 * u + hi5) * E8_OP + j];
        o[u] = (fminf(fmaxf(o[u] - c, -0.5f), 0.5f) + c) * qs[8 * u + hi5];
    }
    inverse8(tab, o, T, X, 128.f);
    store_image8(out, t, w, X);
}

// ------------------------------------------------------------------------------------------------ 16-point tile (the layout of esr_jpeg16.hip)
constexpr int E16_TB = 16;                  // blocks per workgroup along W
constexpr int E16_XB = 20;                  // floats per block of an image row in LDS (16 + 4)
constexpr int E16_XP = E16_TB * E16_XB;     // floats per image row of the tile
constexpr int E16_TR = 16 * E16_TB + 16;    // floats per r of T

// grid: x = tile along w, y = block row, z = image * 2 + plane (Cb, Cr: the last two planes of `desired`)
__global__ __launch_bounds__(ED_THREADS) void pair16_kernel(const float* __restrict__ desired, int img_C, int h, int w, const float* __restrict__ coef,
                                                            int coef_C, int coef_c0, const float* __restrict__ qtab, Dct16Tab tab, int vec,
                                                            float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float X[16 * E16_XP];
    __shared__ __attribute__((aligned(16))) float Q[64 * E16_TB];
    __shared__ float T[16 * E16_TR];
    __shared__ float qs[256];
    const int tid = threadIdx.x, j0 = blockIdx.x * E16_TB, i = blockIdx.y, b = blockIdx.z >> 1, p = blockIdx.z & 1;
    const int nb = min(E16_TB, w - j0);
    const long long W = 16ll * w;
    const float* src = desired + (((long long)b * img_C + img_C - 2 + p) * 16 * h + 16 * i) * W + 16 * j0;
    for (int k = tid; k < 16 * 4 * E16_TB; k += ED_THREADS) {
        const int r = k / (4 * E16_TB), c4 = k % (4 * E16_TB);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < 4 * nb) v = *(const float4*)(src + r * W + 4 * c4);
        *(float4*)(X + r * E16_XP + E16_XB * (c4 >> 2) + 4 * (c4 & 3)) = v;
    }
    {   // the plane's 64 quantised coefficients at the tile's blocks: one group of four per thread
        const int c = tid / (E16_TB / 4), jq = tid % (E16_TB / 4), n = nb - 4 * jq;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        if (n > 0) {
            const float* q = coef + (((long long)b * coef_C + coef_c0 + 64 * p + c) * h + i) * w + j0 + 4 * jq;
            if (vec) {
                const float4 v = *(const float4*)q;
                e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
            } else {
                for (int m = 0; m < 4 && m < n; ++m) e[m] = q[m];
            }
        }
        *(float4*)(Q + c * E16_TB + 4 * jq) = make_float4(e[0], e[1], e[2], e[3]);
    }
    qs[tid] = qtab[((long long)b * 3 + 1 + p) * 256 + tid];
    __syncthreads();
    const int hi = tid >> 4, j = tid & 15;
    {   // row transform: thread (r, j)
        float x[16], t[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a = *(const float4*)(X + hi * E16_XP + E16_XB * j + 4 * q);
            x[4 * q] = a.x; x[4 * q + 1] = a.y; x[4 * q + 2] = a.z; x[4 * q + 3] = a.w;
        }
        dct16<16>(tab, x, t);
#pragma unroll
        for (int v = 0; v < 16; ++v) T[hi * E16_TR + v * E16_TB + j] = t[v];
    }
    __syncthreads();
    {   // column transform, the correction and the inverse column transform: thread (v, j), on the entries T[.][v][j] that no other thread touches
        float t[16], c[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = T[r * E16_TR + hi * E16_TB + j];
        dct16<16>(tab, t, c);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float q = qs[16 * u + hi];
            float s = c[u] / q;
            if (u < 8 && hi < 8) {
                const float k = Q[(8 * u + hi) * E16_TB + j];
                s = fminf(fmaxf(s - k, -0.5f), 0.5f) + k;
            }
            c[u] = s * q;
        }
        idct16<16>(tab, c, t);
#pragma unroll
        for (int r = 0; r < 16; ++r) T[r * E16_TR + hi * E16_TB + j] = t[r];
    }
    __syncthreads();
    {   // inverse row transform: thread (r, j)
        float t[16], x[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) t[v] = T[hi * E16_TR + v * E16_TB + j];
        idct16<16>(tab, t, x);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(float4*)(X + hi * E16_XP + E16_XB * j + 4 * q) = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
    }
    __syncthreads();
    float* dst = out + (((long long)b * 2 + p) * 16 * h + 16 * i) * W + 16 * j0;
    for (int k = tid; k < 16 * 4 * E16_TB; k += ED_THREADS) {
        const int r = k / (4 * E16_TB), c4 = k % (4 * E16_TB);
        if (c4 < 4 * nb) *(float4*)(dst + r * W + 4 * c4) = *(const float4*)(X + r * E16_XP + E16_XB * (c4 >> 2) + 4 * (c4 & 3));
    }
}

// tiles of one 8-point image; false where the shape is refused
bool tiles8(int H, int W, int* h, int* w, int* tiles) {
    if (H <= 0 || W <= 0 || (H & 7) || (W & 7) || (long long)(H / 8) * (W / 8) > 0x7FFFFFFFll - E8_TB) return false;
    *h = H / 8;
    *w = W / 8;
    *tiles = (*h * *w + E8_TB - 1) / E8_TB;
    return true;
}

}  // namespace

extern "C" int esr_ycbcr_rgb(const float* x, int B, int H, int W, float* rgb, esr_stream_t stream) {
    return launch_affine3(x, B, H, W, false, rgb, stream);
}

extern "C" int esr_ycbcr_rgb_grad(const float* d_rgb, int B, int H, int W, float* d_x, esr_stream_t stream) {
    return launch_affine3(d_rgb, B, H, W, true, d_x, stream);
}

extern "C" int64_t esr_jpeg_violation_partials(int H, int W) {
    int h, w, tiles;
    if (!tiles8(H, W, &h, &w, &tiles)) return ESR_E_ARG;
    return tiles;
}

extern "C" int esr_jpeg_violation(const float* cand, int N, int H, int W, const float* coef, int coef_n, const float* qtab, int qtab_n, double* partial,
                                  double* score, esr_stream_t stream) {
    int h, w, tiles;
    if (!cand || !coef || !qtab || !partial || !score || N <= 0 || !tiles8(H, W, &h, &w, &tiles) || !al16(cand) || (coef_n != 1 && coef_n != N) ||
        (qtab_n != 1 && qtab_n != N))
        return ESR_E_ARG;
    if ((long long)N * tiles > 0x7FFFFFFFll) return ESR_E_UNSUPPORTED;
    const int hw = h * w;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(violation_kernel, dim3((unsigned)(N * tiles)), dim3(ED_THREADS), 0, (hipStream_t)stream, cand, h, w, tiles, coef,
                       coef_n == 1 ? 0ll : 64ll * hw, qtab, qtab_n == 1 ? 0 : 64, dct_tab(), coef_vec(hw, coef), partial);
    ESR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)N), dim3(ED_THREADS), 0, (hipStream_t)stream, (const double*)partial, (long long)tiles, score);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_jpeg_pair(const float* desired, int B, int H, int W, const float* coef, const float* qtab, float* out, esr_stream_t stream) {
    int h, w, tiles;
    if (!desired || !coef || !qtab || !out || B <= 0 || !tiles8(H, W, &h, &w, &tiles) || !al16(desired) || !al16(out)) return ESR_E_ARG;
    if ((long long)B * tiles > 0x7FFFFFFFll) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(pair8_kernel, dim3((unsigned)(B * tiles)), dim3(ED_THREADS), 0, (hipStream_t)stream, desired, h, w, tiles, coef, qtab, dct_tab(),
                       coef_vec(h * w, coef), out);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_jpeg16_pair(const float* desired, int desired_C, int B, int H, int W, const float* coef, int coef_C, int coef_c0, const float* qtab,
                               float* out, esr_stream_t stream) {
    if (!desired || !coef || !qtab || !out || B <= 0 || H <= 0 || W <= 0 || (H & 15) || (W & 15) || (desired_C != 2 && desired_C != 3) || coef_c0 < 0 ||
        coef_C < coef_c0 + 128 || !al16(desired) || !al16(out))
        return ESR_E_ARG;
    const int h = H / 16, w = W / 16;
    if (!grid_fits(B, 2, h)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(pair16_kernel, dim3((unsigned)((w + E16_TB - 1) / E16_TB), (unsigned)h, (unsigned)(B * 2)), dim3(ED_THREADS), 0,
                       (hipStream_t)stream, desired, desired_C, h, w, coef, coef_C, coef_c0, qtab, dct16_tab(), coef_vec(w, coef), out);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
