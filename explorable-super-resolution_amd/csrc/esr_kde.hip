// Pairwise KDE kernels behind the patch-histogram and dictionary Z objectives (reference codes/Z_optimization.py:24-230,
// ComputeSoftHistogram :168-209 and Desired_Im_2_Bins :102-125).  Between D-dimensional points x_i (image patches, gray, optionally DC-free) and
// b_j (the desired image's de-duplicated patches, or the 256 gray-level centres) the pair score and kernel value are
//     s_ij = (1/D) sum_d (w(x_id - b_jd) + eps)^2,   w(δ) = min(|δ|, |δ - P|, |δ + P|)   (P = the histogram's `max`, :177-179),
//     k_ij = exp(-s_ij / T).
// The reference materialises [D, N, M] float64 tensors (184 GB for a 512^2 region); these kernels hold nothing of size N x M.  A workgroup of
// 256 threads owns 256 OUTER points, one per thread with its D coordinates in registers, and streams a range of INNER points through LDS in
// chunks of KDE_CH (every lane reads the same inner point: an LDS broadcast).  The per-pair work is plain VALU (sub, sub, add, min3 with |.|
// modifiers, add, fma per dimension): the wrap makes this no GEMM.  P = 1 and |δ| up to 2 (DC-free patches lie in [-1, 1]) is exactly where the
// three-way min and |δ - rint(δ)| differ, so the three-way min is what is computed.
//
// Sums of k run in the log domain — a running maximum m of -s/T and a sum of exp(-s/T - m), rescaled when m grows, fp32 within an LDS chunk and
// folded into a double per chunk (as esr_soft_hist_fwd folds).  At T = 1e-3 two unrelated DC-free patches have s/T ~ 170 and exp(-170) is below
// fp32's range: a plain fp32 sum would give 0 and -log 0 = inf where the reference (float64) is finite.  Where the reference's own float64
// exp underflows (s/T > ~745 for every pair of a row) it returns inf; the log-domain result stays finite — the one intended divergence.
//
//   esr_kde_fwd   per OUTER point o and inner range r: (max_o,r, sum_o,r) with log sum_{inner i in r} k_oi = max + log(sum).  Column mode
//                 (KDE histogram): outer = bins, the ranges = slabs of one image's patches each; row mode (dictionary): outer = patches, the
//                 ranges = slabs of the bins.  The caller folds the ranges (a log-sum-exp over [ranges] per image) in double.
//   esr_kde_bwd   dX[i, d] for outer = patches (tiles of at most 256 rows of ONE image), inner = a slab of bins:
//                     dX[i, d] = sum_j g_i gb_bj exp(-s_ij/T - l_i - lb_bj) * (-2 / (D T)) * (w + eps) * sgn
//                 with sgn the sign of the chosen wrapped difference (wrapped_diff of esr_zobj.hip: negative -> -1, else +1).  Row mode passes
//                 (g_i, l_i) = (upstream gradient, log row sum) and no per-bin arrays: the weights are the softmax k_ij / sum_j k_ij; column mode
//                 passes (gb_bj, lb_bj) = (upstream gradient of log column sum, log column sum) of the tile's image b.  One partial dX per bin
//                 slab, summed by the caller.
//   esr_kde_dedup keep[i] = 0 iff some j > i has |b_id - b_jd| < half_width in every d (Desired_Im_2_Bins with num_sub_images = 1).
#include "esr_common.h"

namespace {

constexpr int KDE_THREADS = 256;
constexpr int KDE_CH = 128;                 // inner points per LDS chunk
constexpr float KDE_EPS = 1e-7f;            // the reference's SQRT_EPSILON

template <int D>
__device__ __forceinline__ float kde_score(const float (&x)[D], const float* __restrict__ b, float P) {
    float a0 = 0.f, a1 = 0.f;              // two chains: latency and a shorter fp32 summation
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float d0 = x[d] - b[d];
        const float w = fminf(fabsf(d0), fminf(fabsf(d0 - P), fabsf(d0 + P)));
        const float t = w + KDE_EPS;
        if (d & 1) a1 = fmaf(t, t, a1);
        else a0 = fmaf(t, t, a0);
    }
    return a0 + a1;
}

template <int D>
__device__ __forceinline__ void kde_stage(float* __restrict__ lds, const float* __restrict__ src, int cnt) {
    for (int t = threadIdx.x; t < cnt * D; t += KDE_THREADS) lds[t] = src[t];
}

template <int D>
__global__ __launch_bounds__(KDE_THREADS) void kde_fwd_kernel(const float* __restrict__ outer, long long n_outer, const float* __restrict__ inner,
                                                              const int* __restrict__ ranges, float P, float scale, float* __restrict__ pmax,
                                                              double* __restrict__ psum) {
    __shared__ float lds[KDE_CH * D];
    const long long o = (long long)blockIdx.x * KDE_THREADS + threadIdx.x;
    const int r0 = ranges[2 * blockIdx.y], r1 = ranges[2 * blockIdx.y + 1];
    const bool live = o < n_outer;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = live ? outer[o * D + d] : 0.f;
    float m = -INFINITY, sf = 0.f;
    double sd = 0.0;
    for (int c0 = r0; c0 < r1; c0 += KDE_CH) {
        const int cnt = min(KDE_CH, r1 - c0);
        __syncthreads();
        kde_stage<D>(lds, inner + (long long)c0 * D, cnt);
        __syncthreads();
        for (int p = 0; p < cnt; ++p) {
            const float e = -kde_score<D>(x, lds + p * D, P) * scale;
            if (e > m) {                    // new maximum: rescale what was summed against the old one
                const float r = __expf(m - e);
                sd *= (double)r;
                sf = fmaf(sf, r, 1.f);
                m = e;
            } else {
                sf += __expf(e - m);
            }
        }
        sd += (double)sf;
        sf = 0.f;
    }
    if (live) {
        const long long k = (long long)blockIdx.y * n_outer + o;
        pmax[k] = m;
        psum[k] = sd;
    }
}

template <int D>
__global__ __launch_bounds__(KDE_THREADS) void kde_bwd_kernel(const float* __restrict__ X, long long R, const int* __restrict__ tiles,
                                                              const float* __restrict__ bins, int M, int bins_per_slab, float P, float scale,
                                                              const float* __restrict__ g_row, const float* __restrict__ l_row,
                                                              const float* __restrict__ g_bin, const float* __restrict__ l_bin, float* __restrict__ dxpart) {
    __shared__ float lds[KDE_CH * D];
    __shared__ float lg[KDE_CH], ll[KDE_CH];
    const int b = tiles[3 * blockIdx.x], t0 = tiles[3 * blockIdx.x + 1], t1 = tiles[3 * blockIdx.x + 2];
    const long long i = (long long)t0 + threadIdx.x;
    const bool live = i < t1;
    const int j0 = blockIdx.y * bins_per_slab, j1 = min(M, j0 + bins_per_slab);
    float x[D], g[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        x[d] = live ? X[i * D + d] : 0.f;
        g[d] = 0.f;
    }
    const float gi = (g_row && live) ? g_row[i] : 1.f;
    const float li = (l_row && live) ? l_row[i] : 0.f;
    const float c = -2.f * scale;
    for (int c0 = j0; c0 < j1; c0 += KDE_CH) {
        const int cnt = min(KDE_CH, j1 - c0);
        __syncthreads();
        kde_stage<D>(lds, bins + (long long)c0 * D, cnt);
        for (int t = threadIdx.x; t < cnt; t += KDE_THREADS) {
            lg[t] = g_bin ? g_bin[(long long)b * M + c0 + t] : 1.f;
            ll[t] = l_bin ? l_bin[(long long)b * M + c0 + t] : 0.f;
        }
        __syncthreads();
        for (int p = 0; p < cnt; ++p) {
            const float* bp = lds + p * D;
            float q[D];
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                // the signed difference among (v - c), (v - c - P), (v - c + P) of smallest magnitude (wrapped_diff, esr_zobj.hip)
                const float d0 = x[d] - bp[d], d1 = d0 - P, d2 = d0 + P;
                float s = d0;
                if (fabsf(d1) < fabsf(s)) s = d1;
                if (fabsf(d2) < fabsf(s)) s = d2;
                const float t = fabsf(s) + KDE_EPS;
                q[d] = s < 0.f ? -t : t;
                if (d & 1) a1 = fmaf(t, t, a1);
                else a0 = fmaf(t, t, a0);
            }
            const float w = gi * lg[p] * __expf(-(a0 + a1) * scale - li - ll[p]) * c;
#pragma unroll
            for (int d = 0; d < D; ++d) g[d] = fmaf(w, q[d], g[d]);
        }
    }
    if (live) {
        float* o = dxpart + ((long long)blockIdx.y * R + i) * D;
#pragma unroll
        for (int d = 0; d < D; ++d) o[d] = g[d];
    }
}

template <int D>
__global__ __launch_bounds__(KDE_THREADS) void kde_dedup_kernel(const float* __restrict__ bins, int M, float half_width, int* __restrict__ keep) {
    __shared__ float lds[KDE_CH * D];
    const int i = blockIdx.x * KDE_THREADS + threadIdx.x;
    const bool live = i < M;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = live ? bins[(long long)i * D + d] : 0.f;
    bool dup = false;
    for (int c0 = blockIdx.x * KDE_THREADS + 1; c0 < M; c0 += KDE_CH) {      // only j > i matter: start after the block's first row
        const int cnt = min(KDE_CH, M - c0);
        __syncthreads();
        kde_stage<D>(lds, bins + (long long)c0 * D, cnt);
        __syncthreads();
        for (int p = 0; p < cnt; ++p) {
            if (c0 + p <= i || dup) continue;
            bool all = true;
#pragma unroll
            for (int d = 0; d < D; ++d) all = all && (fabsf(x[d] - lds[p * D + d]) < half_width);
            dup = all;
        }
    }
    if (live) keep[i] = dup ? 0 : 1;
}

template <int D>
int kde_fwd_launch(const float* outer, long long n_outer, const float* inner, const int* ranges, int n_ranges, float P, float scale, float* pmax,
                   double* psum, hipStream_t s) {
    const dim3 grid((unsigned)((n_outer + KDE_THREADS - 1) / KDE_THREADS), (unsigned)n_ranges);
    hipLaunchKernelGGL(kde_fwd_kernel<D>, grid, dim3(KDE_THREADS), 0, s, outer, n_outer, inner, ranges, P, scale, pmax, psum);
    return ESR_OK;
}

template <int D>
int kde_bwd_launch(const float* X, long long R, const int* tiles, int n_tiles, const float* bins, int M, int bins_per_slab, int n_slabs, float P, float scale,
                   const float* g_row, const float* l_row, const float* g_bin, const float* l_bin, float* dxpart, hipStream_t s) {
    hipLaunchKernelGGL(kde_bwd_kernel<D>, dim3((unsigned)n_tiles, (unsigned)n_slabs), dim3(KDE_THREADS), 0, s, X, R, tiles, bins, M, bins_per_slab, P, scale,
                       g_row, l_row, g_bin, l_bin, dxpart);
    return ESR_OK;
}

template <int D>
int kde_dedup_launch(const float* bins, int M, float half_width, int* keep, hipStream_t s) {
    hipLaunchKernelGGL(kde_dedup_kernel<D>, dim3((unsigned)((M + KDE_THREADS - 1) / KDE_THREADS)), dim3(KDE_THREADS), 0, s, bins, M, half_width, keep);
    return ESR_OK;
}

// the supported point dimensions: gray pixels (1) and square patches of side 2..8
#define KDE_DISPATCH(D_, CALL)        \
    switch (D_) {                     \
        case 1: return CALL(1);       \
        case 4: return CALL(4);       \
        case 9: return CALL(9);       \
        case 16: return CALL(16);     \
        case 25: return CALL(25);     \
        case 36: return CALL(36);     \
        case 49: return CALL(49);     \
        case 64: return CALL(64);     \
        default: return ESR_E_ARG;    \
    }

}  // namespace

extern "C" int esr_kde_dim_supported(int D) { return D == 1 || D == 4 || D == 9 || D == 16 || D == 25 || D == 36 || D == 49 || D == 64; }

extern "C" int esr_kde_fwd(const float* outer, int64_t n_outer, const float* inner, const int32_t* ranges, int n_ranges, int D, float period, float scale,
                           float* pmax, double* psum, esr_stream_t stream) {
    if (!outer || !inner || !ranges || !pmax || !psum || n_outer <= 0 || n_ranges <= 0 || n_ranges > 65535 || !esr_kde_dim_supported(D) || !(scale > 0.f))
        return ESR_E_ARG;
    ESR_CLEAR_ERR();
    int rc;
#define KDE_FWD(D__) kde_fwd_launch<D__>(outer, (long long)n_outer, inner, ranges, n_ranges, period, scale, pmax, psum, (hipStream_t)stream)
    auto go = [&]() -> int { KDE_DISPATCH(D, KDE_FWD) };
#undef KDE_FWD
    rc = go();
    if (rc != ESR_OK) return rc;
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_kde_bwd(const float* X, int64_t R, const int32_t* tiles, int n_tiles, const float* bins, int M, int bins_per_slab, int n_slabs, int D,
                           float period, float scale, const float* g_row, const float* l_row, const float* g_bin, const float* l_bin, float* dxpart,
                           esr_stream_t stream) {
    if (!X || !tiles || !bins || !dxpart || R <= 0 || n_tiles <= 0 || M <= 0 || bins_per_slab <= 0 || n_slabs <= 0 || n_slabs > 65535 ||
        (int64_t)bins_per_slab * n_slabs < M || !esr_kde_dim_supported(D) || !(scale > 0.f) || ((g_bin == nullptr) != (l_bin == nullptr)))
        return ESR_E_ARG;
    ESR_CLEAR_ERR();
#define KDE_BWD(D__) kde_bwd_launch<D__>(X, (long long)R, tiles, n_tiles, bins, M, bins_per_slab, n_slabs, period, scale, g_row, l_row, g_bin, l_bin, dxpart, \
                                         (hipStream_t)stream)
    auto go = [&]() -> int { KDE_DISPATCH(D, KDE_BWD) };
#undef KDE_BWD
    const int rc = go();
    if (rc != ESR_OK) return rc;
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_kde_dedup(const float* bins, int M, int D, float half_width, int32_t* keep, esr_stream_t stream) {
    if (!bins || !keep || M <= 0 || !esr_kde_dim_supported(D)) return ESR_E_ARG;
    ESR_CLEAR_ERR();
#define KDE_DEDUP(D__) kde_dedup_launch<D__>(bins, M, half_width, keep, (hipStream_t)stream)
    auto go = [&]() -> int { KDE_DISPATCH(D, KDE_DEDUP) };
#undef KDE_DEDUP
    const int rc = go();
    if (rc != ESR_OK) return rc;
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
