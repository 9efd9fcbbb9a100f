// Scores of the SR output, on the device: PSNR and SSIM of an image pair and the per-pixel spread over Z samples — what the reference's test.py
// computes in NumPy/OpenCV after copying every image to the host (codes/utils/util.py:196-228 tensor2img, :340-391 calculate_psnr / ssim /
// calculate_ssim; codes/test.py:198-242, :224-233 'stats').
//
// esr_psnr_ssim: one workgroup owns a 21 x 32 tile of one image plane, cropped by `border`.  It converts the tile and a 10-pixel halo below and to
// the right of both images to 0...255 pixels with tensor2img's fp32 arithmetic and keeps them in LDS (fp32 holds them exactly), adds up the squared
// differences of its own 21 x 32 pixels, runs the reference's 11-tap Gaussian horizontally over a, b, a^2, b^2 and ab into fp64 LDS maps and then
// vertically (the window is an outer product: separable), and evaluates the SSIM map at the windows whose top-left corner lies in the tile —
// only windows that fit the cropped image (the reference's [5:-5] crop of filter2D's result).  Everything after the conversion is fp64: E[x^2] - mu^2
// at 0...255 loses 2e-6 of SSIM in fp32.  Each workgroup writes one (squared error, SSIM sum) pair; a second launch adds the pairs of an image in
// a fixed order.  No atomics: two calls give the same bits.  Traffic: each pixel of both images is read once from HBM (the halo re-reads hit L2).
//
// esr_sample_std: one thread owns a pixel, reads its S samples twice (mean, then squared deviations: np.std's two passes) in fp64, writes the fp32
// map and adds the un-rounded value to its workgroup's partial sum; the same second launch adds the partials of an image.
#include "esr_common.h"

#include <cmath>

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_TAPS = 11;                      // cv2.getGaussianKernel(11, 1.5)
constexpr int MT_HALO = MT_TAPS - 1;
constexpr int MT_W = 32, MT_H = 21;              // windows (and owned pixels) per workgroup
constexpr int MT_SW = MT_W + MT_HALO, MT_SH = MT_H + MT_HALO;
constexpr int MT_CB = 4, MT_RB = 3;              // windows per thread: columns in the horizontal pass, rows in the vertical pass
constexpr int MT_PS = MT_SW + 1, MT_MS = MT_W + 1;      // LDS row strides: the horizontal pass reads pixels 4 columns apart and writes moments likewise
static_assert(MT_SH * (MT_W / MT_CB) <= MT_THREADS && (MT_H / MT_RB) * MT_W <= MT_THREADS && MT_W % MT_CB == 0 && MT_H % MT_RB == 0, "one item per thread");
constexpr int MT_STAGE = (MT_SH * MT_SW + MT_THREADS - 1) / MT_THREADS;      // staged pixels per thread
constexpr int SS_PIXELS = 1024;                  // pixels per workgroup of esr_sample_std

struct Gauss11 { double w[MT_TAPS]; };

// tensor2img (utils/util.py:224-226) in fp32: (clip(x, lo, hi) - lo) / (hi - lo), times 255, .round() (half to even) for uint8
__device__ __forceinline__ float to_pixel(float x, float lo, float hi, float den, int mode) {
    if (mode == ESR_PIXELS_RAW) return x;
    const float v = __fdiv_rn(fminf(fmaxf(x, lo), hi) - lo, den);
    const float p = v * 255.f;
    return mode == ESR_PIXELS_ROUND ? rintf(p) : p;
}

// sum of v[] over the workgroup, in thread 0, in a fixed order: lanes by shuffles, then the waves one after the other
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] += __shfl_down(v[j], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int j = 0; j < N; ++j) red[wave * N + j] = v[j];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < MT_WAVES; ++w)
            for (int j = 0; j < N; ++j) v[j] += red[w * N + j];
}

__global__ __launch_bounds__(MT_THREADS) void psnr_ssim_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W, float lo, float hi,
                                                               int mode, int border, Gauss11 g, double* __restrict__ partial) {
    __shared__ float pa[MT_SH][MT_PS], pb[MT_SH][MT_PS];
    __shared__ double hm[5][MT_SH][MT_MS];
    __shared__ double red[MT_WAVES * 2];
    const int tid = threadIdx.x;
    const int Hc = H - 2 * border, Wc = W - 2 * border;
    const int x0 = blockIdx.x * MT_W, y0 = blockIdx.y * MT_H;                       // the tile's origin in the cropped plane
    const long long origin = (long long)blockIdx.z * H * W + (long long)border * W + border;
    const float den = hi - lo;
    double acc[2] = {0.0, 0.0};                                                      // squared error, SSIM sum

    // stage the tile and its halo: every load is issued before the first conversion (a workgroup has few waves to hide their latency behind)
    float xa[MT_STAGE], xb[MT_STAGE];
#pragma unroll
    for (int it = 0; it < MT_STAGE; ++it) {
        const int i = tid + it * MT_THREADS, r = i / MT_SW, c = i % MT_SW;
        const bool in = i < MT_SH * MT_SW && y0 + r < Hc && x0 + c < Wc;
        const long long o = origin + (long long)(y0 + r) * W + (x0 + c);
        xa[it] = in ? a[o] : 0.f;
        xb[it] = in ? b[o] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < MT_STAGE; ++it) {
        const int i = tid + it * MT_THREADS, r = i / MT_SW, c = i % MT_SW;
        if (i >= MT_SH * MT_SW) break;
        const bool in = y0 + r < Hc && x0 + c < Wc;
        const float va = in ? to_pixel(xa[it], lo, hi, den, mode) : 0.f, vb = in ? to_pixel(xb[it], lo, hi, den, mode) : 0.f;
        if (in && r < MT_H && c < MT_W) {
            const double d = (double)va - (double)vb;
            acc[0] += d * d;
        }
        pa[r][c] = va;
        pb[r][c] = vb;
    }
    __syncthreads();

    // windows whose corner this tile owns (none along an axis where fewer than 11 pixels are left)
    const int nwx = min(MT_W, Wc - MT_HALO - x0), nwy = min(MT_H, Hc - MT_HALO - y0);
    if (nwx > 0 && nwy > 0) {                                                        // uniform over the workgroup
        // horizontal pass: a thread owns MT_CB adjacent columns of one staged row, so a pixel and its three products are read and formed once
        // for up to MT_CB windows (taps in ascending order for every output)
        if (tid < MT_SH * (MT_W / MT_CB)) {
            const int r = tid / (MT_W / MT_CB), c0 = (tid % (MT_W / MT_CB)) * MT_CB;
            double s[MT_CB][5] = {};
#pragma unroll
            for (int k = 0; k < MT_CB + MT_HALO; ++k) {
                const double u = (double)pa[r][c0 + k], v = (double)pb[r][c0 + k];
                const double p[5] = {u, v, u * u, v * v, u * v};
#pragma unroll
                for (int j = 0; j < MT_CB; ++j)
                    if (k - j >= 0 && k - j < MT_TAPS)
#pragma unroll
                        for (int m = 0; m < 5; ++m) s[j][m] += g.w[k - j] * p[m];
            }
#pragma unroll
            for (int j = 0; j < MT_CB; ++j)
#pragma unroll
                for (int m = 0; m < 5; ++m) hm[m][r][c0 + j] = s[j][m];
        }
        __syncthreads();
        // vertical pass: a thread owns MT_RB adjacent rows of one column
        constexpr double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
        if (tid < (MT_H / MT_RB) * MT_W) {
            const int c = tid % MT_W, r0 = (tid / MT_W) * MT_RB;
            double s[MT_RB][5] = {};
#pragma unroll
            for (int k = 0; k < MT_RB + MT_HALO; ++k) {
                double h[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) h[m] = hm[m][r0 + k][c];
#pragma unroll
                for (int j = 0; j < MT_RB; ++j)
                    if (k - j >= 0 && k - j < MT_TAPS)
#pragma unroll
                        for (int m = 0; m < 5; ++m) s[j][m] += g.w[k - j] * h[m];
            }
#pragma unroll
            for (int j = 0; j < MT_RB; ++j) {
                if (r0 + j >= nwy || c >= nwx) continue;
                const double mu1_sq = s[j][0] * s[j][0], mu2_sq = s[j][1] * s[j][1], mu1_mu2 = s[j][0] * s[j][1];
                const double sigma1_sq = s[j][2] - mu1_sq, sigma2_sq = s[j][3] - mu2_sq, sigma12 = s[j][4] - mu1_mu2;
                acc[1] += ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2));
            }
        }
    }
    block_sum(acc, red);
    if (tid == 0) {
        const long long wg = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * wg] = acc[0];
        partial[2 * wg + 1] = acc[1];
    }
}

// out[b][j] = sum_i partial[b][i][j], i < n, j < WIDTH: thread t adds i = t, t + 256, ... in order, then block_sum
template <int WIDTH>
__global__ __launch_bounds__(MT_THREADS) void sum_partials_kernel(const double* __restrict__ partial, long long n, double* __restrict__ out) {
    __shared__ double red[MT_WAVES * WIDTH];
    const double* p = partial + (long long)blockIdx.x * n * WIDTH;
    double v[WIDTH];
    for (int j = 0; j < WIDTH; ++j) v[j] = 0.0;
    for (long long i = threadIdx.x; i < n; i += MT_THREADS)
        for (int j = 0; j < WIDTH; ++j) v[j] += p[i * WIDTH + j];
    block_sum(v, red);
    if (threadIdx.x == 0)
        for (int j = 0; j < WIDTH; ++j) out[(long long)blockIdx.x * WIDTH + j] = v[j];
}

__global__ __launch_bounds__(MT_THREADS) void sample_std_kernel(const float* __restrict__ x, int S, long long n, float* __restrict__ map,
                                                                double* __restrict__ partial) {
    __shared__ double red[MT_WAVES];
    const long long image = (long long)blockIdx.y * n, sample = (long long)gridDim.y * n;
    double acc[1] = {0.0};
    for (int j = 0; j < SS_PIXELS / MT_THREADS; ++j) {
        const long long i = (long long)blockIdx.x * SS_PIXELS + j * MT_THREADS + threadIdx.x;
        if (i >= n) break;
        const float* p = x + image + i;
        double mean = 0.0;
        for (int s = 0; s < S; ++s) mean += (double)clamp_unit(p[s * sample]);
        mean /= (double)S;
        double q = 0.0;
        for (int s = 0; s < S; ++s) {
            const double d = (double)clamp_unit(p[s * sample]) - mean;
            q += d * d;
        }
        const double sd = 255.0 * sqrt(q / (double)S);
        map[image + i] = (float)sd;
        acc[0] += sd;
    }
    block_sum(acc, red);
    if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

struct MetricsGrid { int gx, gy; };
// the tiles of one cropped plane; false where the shape is refused
static bool metrics_grid(int C, int H, int W, int border, MetricsGrid& t) {
    if ((C != 1 && C != 3) || H < 1 || W < 1 || border < 0 || H - 2 * (long long)border < 1 || W - 2 * (long long)border < 1) return false;
    t.gx = (W - 2 * border + MT_W - 1) / MT_W;
    t.gy = (H - 2 * border + MT_H - 1) / MT_H;
    return true;
}

}  // namespace

extern "C" int64_t esr_psnr_ssim_partials(int C, int H, int W, int border) {
    MetricsGrid t;
    if (!metrics_grid(C, H, W, border, t)) return ESR_E_ARG;
    return (int64_t)C * t.gy * t.gx;
}

extern "C" int esr_psnr_ssim(const float* a, const float* b, int B, int C, int H, int W, float lo, float hi, int quantize, int border, double* partial,
                             double* sums, esr_stream_t stream) {
    MetricsGrid t;
    if (!a || !b || !partial || !sums || B < 1 || !metrics_grid(C, H, W, border, t)) return ESR_E_ARG;
    if (quantize != ESR_PIXELS_FLOAT && quantize != ESR_PIXELS_ROUND && quantize != ESR_PIXELS_RAW) return ESR_E_ARG;
    if (quantize != ESR_PIXELS_RAW && !(hi > lo)) return ESR_E_ARG;
    if ((long long)B * C > 65535 || t.gy > 65535) return ESR_E_UNSUPPORTED;
    Gauss11 g;
    double total = 0.0;
    for (int i = 0; i < MT_TAPS; ++i) {
        g.w[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        total += g.w[i];
    }
    for (int i = 0; i < MT_TAPS; ++i) g.w[i] /= total;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(psnr_ssim_kernel, dim3(t.gx, t.gy, B * C), dim3(MT_THREADS), 0, (hipStream_t)stream, a, b, H, W, lo, hi, quantize, border, g, partial);
    ESR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_partials_kernel<2>, dim3(B), dim3(MT_THREADS), 0, (hipStream_t)stream, (const double*)partial, (long long)C * t.gy * t.gx, sums);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int64_t esr_sample_std_partials(int C, int H, int W) {
    if (C < 1 || H < 1 || W < 1) return ESR_E_ARG;
    return ((int64_t)C * H * W + SS_PIXELS - 1) / SS_PIXELS;
}

extern "C" int esr_sample_std(const float* x, int S, int B, int C, int H, int W, float* map, double* partial, double* sums, esr_stream_t stream) {
    if (!x || !map || !partial || !sums || S < 1 || B < 1 || C < 1 || H < 1 || W < 1) return ESR_E_ARG;
    const long long n = (long long)C * H * W, blocks = (n + SS_PIXELS - 1) / SS_PIXELS;
    if (B > 65535 || blocks > 0x7FFFFFFFll) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(sample_std_kernel, dim3((unsigned)blocks, B), dim3(MT_THREADS), 0, (hipStream_t)stream, x, S, n, map, partial);
    ESR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_partials_kernel<1>, dim3(B), dim3(MT_THREADS), 0, (hipStream_t)stream, (const double*)partial, blocks, sums);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
