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
//
// The JPEG decoder's outputs (Y or YCbCr in 0...255; codes/test_JPEG.py:165-327) are scored by the same kernels behind another pixel source:
// ycbcr_pixel below is tensor2img's chroma branch (utils/util.py:209-226 through data/util.py:198-215) for one output channel of one pixel, in the
// rounding order include/esr_hip.h states.  esr_psnr_ssim_ycbcr stages channel j of both operands through it (a workgroup reads the 1 or 3 input
// planes and keeps one converted value: no converted image is written); esr_sample_std_ycbcr takes np.std of the rounded pixels; esr_ycbcr_image
// writes the uint8 BGR picture, 3 bytes per pixel instead of the 12 of an fp32 copy.
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

// tensor2img's chroma branch for output channel j (0 R, 1 G, 2 B) of one pixel of a C-plane input in 0...255 — the chain of include/esr_hip.h: fp32
// / 255 and x 255, the matrix row and offset in fp64 with every product and sum rounded on its own (contraction is switched off for this function:
// hipcc fuses a * b + c by default, and the *_rn intrinsics do not stop it), one rounding to fp32, x 255 in fp32, then to_pixel.  C = 1 ('Y'):
// both chroma values are the reference's 128 / 255 * np.ones_like(img) in fp32, x 255 (cb and cr are not read).
template <int C>
__device__ __forceinline__ float ycbcr_pixel(float y, float cb, float cr, int j, float lo, float hi, float den, int mode) {
#pragma clang fp contract(off)
    constexpr double M[3][3] = {{0.00456621, 0.00456621, 0.00456621}, {0.0, -0.00153632, 0.00791071}, {0.00625893, -0.00318811, 0.0}};
    constexpr double OFF[3] = {-222.921, 135.576, -276.836};
    constexpr float GREY = (float)(128.0 / 255.0);
    const double x0 = (double)__fmul_rn(__fdiv_rn(y, 255.f), 255.f);
    const double x1 = (double)__fmul_rn(C == 3 ? __fdiv_rn(cb, 255.f) : GREY, 255.f), x2 = (double)__fmul_rn(C == 3 ? __fdiv_rn(cr, 255.f) : GREY, 255.f);
    const double m0 = j == 0 ? M[0][0] : j == 1 ? M[0][1] : M[0][2], m1 = j == 0 ? M[1][0] : j == 1 ? M[1][1] : M[1][2],
                 m2 = j == 0 ? M[2][0] : j == 1 ? M[2][1] : M[2][2], off = j == 0 ? OFF[0] : j == 1 ? OFF[1] : OFF[2];
    const double r = ((x0 * m0 + x1 * m1) + x2 * m2) * 255.0 + off;
    const float q = (float)(r / 255.0);
    return to_pixel(255.f * q, lo, hi, den, mode);
}

// Where the tile kernel's pixels come from.  A source names the planes a workgroup (blockIdx.z) reads per operand and turns the values read at
// one position into the two pixels.  PlaneSource: plane z of a and of b through to_pixel — esr_psnr_ssim.
struct PlaneSource {
    static constexpr int PLANES = 1;
    const float* __restrict__ a;
    const float* __restrict__ b;
    float lo, hi;
    int mode;
    __device__ __forceinline__ void bases(int z, long long hw, const float*& pa, const float*& pb) const {
        pa = a + (long long)z * hw;
        pb = b + (long long)z * hw;
    }
    __device__ __forceinline__ float pixel(const float (&v)[PLANES], int z, float den) const { return to_pixel(v[0], lo, hi, den, mode); }
};
// YcbcrSource<C>: workgroup z scores output channel z % 3 of image z / 3; it reads the C input planes of both operands (operand b with its own
// batch stride: 0 scores every image of a against one ground truth) — esr_psnr_ssim_ycbcr.
template <int C>
struct YcbcrSource {
    static constexpr int PLANES = C;
    const float* __restrict__ a;
    const float* __restrict__ b;
    long long b_stride;
    float lo, hi;
    __device__ __forceinline__ void bases(int z, long long hw, const float*& pa, const float*& pb) const {
        pa = a + (long long)(z / 3) * C * hw;
        pb = b + (long long)(z / 3) * b_stride;
    }
    __device__ __forceinline__ float pixel(const float (&v)[PLANES], int z, float den) const {
        constexpr int CB = C == 3 ? 1 : 0, CR = C == 3 ? 2 : 0;                 // (one plane: cb and cr are not read)
        return ycbcr_pixel<C>(v[0], v[CB], v[CR], z % 3, lo, hi, den, ESR_PIXELS_ROUND);
    }
};

template <class Source>
__global__ __launch_bounds__(MT_THREADS) void psnr_ssim_kernel(Source src, int H, int W, int border, Gauss11 g, double* __restrict__ partial) {
    constexpr int NP = Source::PLANES;
    __shared__ float pa[MT_SH][MT_PS], pb[MT_SH][MT_PS];
    __shared__ double hm[5][MT_SH][MT_MS];
    __shared__ double red[MT_WAVES * 2];
    const int tid = threadIdx.x;
    const int Hc = H - 2 * border, Wc = W - 2 * border;
    const int x0 = blockIdx.x * MT_W, y0 = blockIdx.y * MT_H;                       // the tile's origin in the cropped plane
    const long long hw = (long long)H * W, origin = (long long)border * W + border;
    const float den = src.hi - src.lo;
    const float *ga, *gb;
    src.bases(blockIdx.z, hw, ga, gb);
    double acc[2] = {0.0, 0.0};                                                      // squared error, SSIM sum

    // stage the tile and its halo: every load is issued before the first conversion (a workgroup has few waves to hide their latency behind)
    float xa[MT_STAGE][NP], xb[MT_STAGE][NP];
#pragma unroll
    for (int it = 0; it < MT_STAGE; ++it) {
        const int i = tid + it * MT_THREADS, r = i / MT_SW, c = i % MT_SW;
        const bool in = i < MT_SH * MT_SW && y0 + r < Hc && x0 + c < Wc;
        const long long o = origin + (long long)(y0 + r) * W + (x0 + c);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            xa[it][p] = in ? ga[p * hw + o] : 0.f;
            xb[it][p] = in ? gb[p * hw + o] : 0.f;
        }
    }
#pragma unroll
    for (int it = 0; it < MT_STAGE; ++it) {
        const int i = tid + it * MT_THREADS, r = i / MT_SW, c = i % MT_SW;
        if (i >= MT_SH * MT_SW) break;
        const bool in = y0 + r < Hc && x0 + c < Wc;
        const float va = in ? src.pixel(xa[it], blockIdx.z, den) : 0.f, vb = in ? src.pixel(xb[it], blockIdx.z, den) : 0.f;
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

// esr_sample_std_ycbcr: one thread owns a pixel and its three output channels; the S samples are converted in both passes (nothing is held)
template <int C>
__global__ __launch_bounds__(MT_THREADS) void sample_std_ycbcr_kernel(const float* __restrict__ x, int S, long long hw, float lo, float hi,
                                                                      float* __restrict__ map, double* __restrict__ partial) {
    __shared__ double red[MT_WAVES];
    const long long sample = (long long)gridDim.y * C * hw;
    const float den = hi - lo;
    double acc[1] = {0.0};
    for (int k = 0; k < SS_PIXELS / MT_THREADS; ++k) {
        const long long i = (long long)blockIdx.x * SS_PIXELS + k * MT_THREADS + threadIdx.x;
        if (i >= hw) break;
        const float* p = x + (long long)blockIdx.y * C * hw + i;
        double mean[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
        for (int pass = 0; pass < 2; ++pass) {
            for (int s = 0; s < S; ++s) {
                const float* ps = p + s * sample;
                const float y = ps[0], cb = C == 3 ? ps[hw] : 0.f, cr = C == 3 ? ps[2 * hw] : 0.f;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double v = (double)ycbcr_pixel<C>(y, cb, cr, j, lo, hi, den, ESR_PIXELS_ROUND);
                    if (pass == 0) {
                        mean[j] += v;
                    } else {
                        const double d = v - mean[j];
                        q[j] += d * d;
                    }
                }
            }
            if (pass == 0)
                for (int j = 0; j < 3; ++j) mean[j] /= (double)S;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double sd = sqrt(q[j] / (double)S);
            map[((long long)blockIdx.y * 3 + j) * hw + i] = (float)sd;
            acc[0] += sd;
        }
    }
    block_sum(acc, red);
    if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// esr_ycbcr_image: a thread owns PX adjacent pixels of a row-major image (4 where W % 4 == 0: one 16-byte read per plane, three whole dwords
// out; 1 otherwise: three bytes out).  out is HWC in B, G, R order.
template <int C, int PX>
__global__ __launch_bounds__(MT_THREADS) void ycbcr_image_kernel(const float* __restrict__ x, long long hw, long long groups, float lo, float hi,
                                                                 uint8_t* __restrict__ out) {
    const long long t = (long long)blockIdx.x * MT_THREADS + threadIdx.x;        // group t of image blockIdx.y
    if (t >= groups) return;
    const float den = hi - lo;
    const float* p = x + (long long)blockIdx.y * C * hw + t * PX;
    float v[C][PX];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (PX == 4) {
            const float4 f = *reinterpret_cast<const float4*>(p + c * hw);
            v[c][0] = f.x, v[c][1] = f.y, v[c][2] = f.z, v[c][3] = f.w;
        } else {
            v[c][0] = p[c * hw];
        }
    }
    constexpr int CB = C == 3 ? 1 : 0, CR = C == 3 ? 2 : 0;                     // (one plane: cb and cr are not read)
    uint8_t px[3 * PX];
#pragma unroll
    for (int k = 0; k < PX; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j)           // 0...255 after the clip, B first
            px[3 * k + 2 - j] = (uint8_t)ycbcr_pixel<C>(v[0][k], v[CB][k], v[CR][k], j, lo, hi, den, ESR_PIXELS_ROUND);
    uint8_t* o = out + ((long long)blockIdx.y * hw + t * PX) * 3;
    if constexpr (PX == 4) {
        unsigned* o32 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int d = 0; d < 3; ++d)
            o32[d] = (unsigned)px[4 * d] | (unsigned)px[4 * d + 1] << 8 | (unsigned)px[4 * d + 2] << 16 | (unsigned)px[4 * d + 3] << 24;
    } else {
        o[0] = px[0], o[1] = px[1], o[2] = px[2];
    }
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

static Gauss11 gauss11() {
    Gauss11 g;
    double total = 0.0;
    for (int i = 0; i < MT_TAPS; ++i) {
        g.w[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        total += g.w[i];
    }
    for (int i = 0; i < MT_TAPS; ++i) g.w[i] /= total;
    return g;
}

// the tile launch over `planes` planes per image and the fixed-order sum of every image's partial pairs
template <class Source>
static int launch_psnr_ssim(const Source& src, const MetricsGrid& t, int B, int planes, int H, int W, int border, double* partial, double* sums,
                            esr_stream_t stream) {
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(psnr_ssim_kernel<Source>, dim3(t.gx, t.gy, B * planes), dim3(MT_THREADS), 0, (hipStream_t)stream, src, H, W, border, gauss11(), partial);
    ESR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_partials_kernel<2>, dim3(B), dim3(MT_THREADS), 0, (hipStream_t)stream, (const double*)partial, (long long)planes * t.gy * t.gx, sums);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_psnr_ssim(const float* a, const float* b, int B, int C, int H, int W, float lo, float hi, int quantize, int border, double* partial,
                             double* sums, esr_stream_t stream) {
    MetricsGrid t;
    if (!a || !b || !partial || !sums || B < 1 || !metrics_grid(C, H, W, border, t)) return ESR_E_ARG;
    if (quantize != ESR_PIXELS_FLOAT && quantize != ESR_PIXELS_ROUND && quantize != ESR_PIXELS_RAW) return ESR_E_ARG;
    if (quantize != ESR_PIXELS_RAW && !(hi > lo)) return ESR_E_ARG;
    if ((long long)B * C > 65535 || t.gy > 65535) return ESR_E_UNSUPPORTED;
    return launch_psnr_ssim(PlaneSource{a, b, lo, hi, quantize}, t, B, C, H, W, border, partial, sums, stream);
}

extern "C" int64_t esr_psnr_ssim_ycbcr_partials(int C, int H, int W, int border) {
    MetricsGrid t;
    if (!metrics_grid(C, H, W, border, t)) return ESR_E_ARG;
    return (int64_t)3 * t.gy * t.gx;
}

extern "C" int esr_psnr_ssim_ycbcr(const float* a, const float* b, int B, int C, int H, int W, int64_t b_batch_stride, float lo, float hi, int border,
                                   double* partial, double* sums, esr_stream_t stream) {
    MetricsGrid t;
    if (!a || !b || !partial || !sums || B < 1 || !metrics_grid(C, H, W, border, t) || !(hi > lo)) return ESR_E_ARG;
    if (b_batch_stride != 0 && b_batch_stride != (int64_t)C * H * W) return ESR_E_ARG;
    if ((long long)B * 3 > 65535 || t.gy > 65535) return ESR_E_UNSUPPORTED;
    if (C == 3) return launch_psnr_ssim(YcbcrSource<3>{a, b, (long long)b_batch_stride, lo, hi}, t, B, 3, H, W, border, partial, sums, stream);
    return launch_psnr_ssim(YcbcrSource<1>{a, b, (long long)b_batch_stride, lo, hi}, t, B, 3, H, W, border, partial, sums, stream);
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

extern "C" int64_t esr_sample_std_ycbcr_partials(int C, int H, int W) {
    if ((C != 1 && C != 3) || H < 1 || W < 1) return ESR_E_ARG;
    return ((int64_t)H * W + SS_PIXELS - 1) / SS_PIXELS;
}

extern "C" int esr_sample_std_ycbcr(const float* x, int S, int B, int C, int H, int W, float lo, float hi, float* map, double* partial, double* sums,
                                    esr_stream_t stream) {
    if (!x || !map || !partial || !sums || S < 1 || B < 1 || (C != 1 && C != 3) || H < 1 || W < 1 || !(hi > lo)) return ESR_E_ARG;
    const long long hw = (long long)H * W, blocks = (hw + SS_PIXELS - 1) / SS_PIXELS;
    if (B > 65535 || blocks > 0x7FFFFFFFll) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    if (C == 3)
        hipLaunchKernelGGL(sample_std_ycbcr_kernel<3>, dim3((unsigned)blocks, B), dim3(MT_THREADS), 0, (hipStream_t)stream, x, S, hw, lo, hi, map, partial);
    else
        hipLaunchKernelGGL(sample_std_ycbcr_kernel<1>, dim3((unsigned)blocks, B), dim3(MT_THREADS), 0, (hipStream_t)stream, x, S, hw, lo, hi, map, partial);
    ESR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_partials_kernel<1>, dim3(B), dim3(MT_THREADS), 0, (hipStream_t)stream, (const double*)partial, blocks, sums);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_ycbcr_image(const float* x, int B, int C, int H, int W, float lo, float hi, uint8_t* out, esr_stream_t stream) {
    if (!x || !out || B < 1 || (C != 1 && C != 3) || H < 1 || W < 1 || !(hi > lo)) return ESR_E_ARG;
    const long long hw = (long long)H * W;
    // four pixels per thread need rows of whole groups and aligned bases: 16 bytes for the planes (hw is then a multiple of 4), 4 for the picture
    const bool wide = W % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)out % 4 == 0;
    const long long groups = wide ? hw / 4 : hw, blocks = (groups + MT_THREADS - 1) / MT_THREADS;
    if (B > 65535 || blocks > 0x7FFFFFFFll) return ESR_E_UNSUPPORTED;
    const dim3 grid((unsigned)blocks, B), block(MT_THREADS);
    ESR_CLEAR_ERR();
    if (C == 3 && wide) hipLaunchKernelGGL((ycbcr_image_kernel<3, 4>), grid, block, 0, (hipStream_t)stream, x, hw, groups, lo, hi, out);
    else if (C == 3) hipLaunchKernelGGL((ycbcr_image_kernel<3, 1>), grid, block, 0, (hipStream_t)stream, x, hw, groups, lo, hi, out);
    else if (wide) hipLaunchKernelGGL((ycbcr_image_kernel<1, 4>), grid, block, 0, (hipStream_t)stream, x, hw, groups, lo, hi, out);
    else hipLaunchKernelGGL((ycbcr_image_kernel<1, 1>), grid, block, 0, (hipStream_t)stream, x, hw, groups, lo, hi, out);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
