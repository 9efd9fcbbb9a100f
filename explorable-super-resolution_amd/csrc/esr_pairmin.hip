// Random-alternatives Z objective (reference codes/Z_optimization.py:683-701): the term behind the GUI's "produce random alternatives" tool,
// the one objective that couples the samples of a batch.  With I_r = clamp(x_r, 0, 1) (clamp01) or x_r (feature tensors), per element
// e = (c, h, w) and row r of the GLOBAL batch x [Bg][C][H][W]:
//     d(r, a)  = |I_r - I_a| for a != r,   d(r, r) = 1                      (the reference's "+ eye" diagonal)
//     a*(r)    = the LOWEST index a with d(r, a) = min_a d(r, a)            (an exact tie goes to the lowest index, the diagonal included as
//                                                                             index r; torch.min leaves the choice open)
//     v(r, e)  = m(h, w) (d(r, a*(r)) - w |I_r - init_r|)                   (m: the optional image mask; the second term with `init` only)
// The reference builds d as a [Bg][Bg][C][H][W] tensor (12.9 GB at 64 x 3 x 512^2); here a thread owns one element, keeps the Bg values of that
// element in a private LDS column (vals[a][thread]) and walks the rows in register tiles of 16, so nothing of size Bg x Bg exists anywhere.
// The column holds x as it is: the clamp is applied where a value is read (one v_med3), and the backward finds its gate beside the value.
// Forward (esr_pairmin): the rows [lo, hi) only.  partial[r - lo][block] = sum over the block's elements of v(r, e): per-element floats, summed
//   in double over a wave (fixed shuffle tree), over the block's chunks and over its waves in a fixed order.  The caller sums the blocks.  No
//   atomics: two runs are bit-identical.
// Backward (esr_pairmin_grad), gather form: dx[b - lo][e] = scale m(h, w) gate(x_b) (sum_{r != b, a*(r) = b} sign(I_b - I_r)
//   + [a*(b) != b] sign(I_b - I_a*(b)) - w sign(I_b - init_b)) for the local rows b, where r runs over ALL Bg rows (the rows of other ranks
//   that chose b as their nearest neighbour count), sign(0) = 0 and gate = [0 <= x_b <= 1] with clamp01, 1 without.  The thread that owns the
//   element adds every row's two terms into its own column of a second LDS array and then writes its own outputs: no scatter to memory, no atomics.
// Batches whose columns do not fit in 160 KiB of LDS (about 300 rows forward; Bg + hi - lo > 320 backward) take the same code with the columns
// in global memory (`work`, and dx itself as the accumulator): any Bg >= 1 runs.
#include "esr_image.h"

namespace {

constexpr int P_THREADS = 128;      // one element per thread: vals[Bg][128] is 32 KiB at Bg = 64
constexpr int P_TILE = 16;          // rows held in registers while the column is walked once
constexpr int P_MAX_BLOCKS = 4096;
constexpr size_t P_LDS_LIMIT = 160 * 1024;

// the columns hold x as it is: the clamp is one v_med3 per read, and the backward finds its gate [0 <= x <= 1] next to the value
__device__ __forceinline__ float rd(float v, bool clamp) { return clamp ? __builtin_amdgcn_fmed3f(v, 0.f, 1.f) : v; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct PairArgs {
    const float* x;          // [Bg][n]
    const float* mask;       // [hw] or null
    const float* init;       // [init_batch][n] or null
    long long n, hw;         // elements per row (C H W), pixels per plane (H W)
    int Bg, lo, hi, clamp01, init_batch;
    float w;
};

// the column of element e: vals[a * stride + col] for a in [0, Bg).  LDS: stride = P_THREADS, col = threadIdx.x; global: stride = n, col = e.
template <bool GRAD, typename VP>
__device__ __forceinline__ void walk_tile(const VP vals, long long stride, long long col, bool clamp, int Bg, int r0, int r1, float (&sd)[P_TILE],
                                          int (&arg)[P_TILE]) {
    // sd: the winning difference I_r - I_a, signed (GRAD; 1 when the diagonal won) or its magnitude (forward); arg: the winner (GRAD only)
    float vr[P_TILE];
#pragma unroll
    for (int k = 0; k < P_TILE; ++k) {
        vr[k] = r0 + k < r1 ? rd(vals[(long long)(r0 + k) * stride + col], clamp) : 0.f;
        sd[k] = INFINITY;
        arg[k] = -1;
    }
    // a strict `<` in increasing a keeps the lowest index on a tie; the diagonal takes its turn at a = r with distance 1.  Three stretches of a
    // (below the tile, inside it, above it) so that only the 16 steps inside the tile pay for the diagonal's compare
    auto step = [&](int a, bool diag) {
        const float va = rd(vals[(long long)a * stride + col], clamp);
#pragma unroll
        for (int k = 0; k < P_TILE; ++k) {
            float d = vr[k] - va;
            if (diag && a == r0 + k) d = 1.f;
            if (GRAD) {
                const bool t = fabsf(d) < fabsf(sd[k]);
                sd[k] = t ? d : sd[k];
                arg[k] = t ? a : arg[k];
            } else {
                sd[k] = fminf(sd[k], fabsf(d));
            }
        }
    };
    const int t1 = r0 + P_TILE < Bg ? r0 + P_TILE : Bg;
#pragma unroll 4
    for (int a = 0; a < r0; ++a) step(a, false);
    for (int a = r0; a < t1; ++a) step(a, true);
#pragma unroll 4
    for (int a = t1; a < Bg; ++a) step(a, false);
}

template <bool LDS>
__global__ __launch_bounds__(P_THREADS) void pairmin_kernel(PairArgs p, float* __restrict__ work, double* __restrict__ partial) {
    extern __shared__ __align__(16) float smem[];
    const int nl = p.hi - p.lo;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long chunks = (p.n + P_THREADS - 1) / P_THREADS;
    // per-thread running sums would need a register per row: the block keeps one double per (wave, row) in LDS instead, owned by lane 0 of the wave
    double* rows = reinterpret_cast<double*>(smem + (LDS ? (size_t)p.Bg * P_THREADS : 0));       // [waves][nl]
    for (int i = threadIdx.x; i < (P_THREADS / 64) * nl; i += P_THREADS) rows[i] = 0.0;
    __syncthreads();
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const long long e = ch * P_THREADS + threadIdx.x;
        const bool live = e < p.n;
        const long long stride = LDS ? P_THREADS : p.n, col = LDS ? threadIdx.x : (live ? e : 0);
        float* vals = LDS ? smem : work;
        if (live)
            for (int a = 0; a < p.Bg; ++a) vals[(long long)a * stride + col] = p.x[(long long)a * p.n + e];
        const float m = !live ? 0.f : (p.mask ? p.mask[e % p.hw] : 1.f);
        for (int r0 = p.lo; r0 < p.hi; r0 += P_TILE) {
            float sd[P_TILE];
            int arg[P_TILE];
            if (live) walk_tile<false>(vals, stride, col, p.clamp01 != 0, p.Bg, r0, p.hi, sd, arg);
#pragma unroll
            for (int k = 0; k < P_TILE; ++k) {
                if (r0 + k >= p.hi) break;                                   // (uniform over the block)
                float v = 0.f;
                if (live) {
                    v = sd[k];
                    if (p.init) {
                        const float vr = rd(vals[(long long)(r0 + k) * stride + col], p.clamp01 != 0);
                        v -= p.w * fabsf(vr - p.init[(p.init_batch == 1 ? 0 : (long long)(r0 + k - p.lo)) * p.n + e]);
                    }
                    v *= m;
                }
                const double s = wave_sum((double)v);
                if (lane == 0) rows[wave * nl + (r0 + k - p.lo)] += s;
            }
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < nl; r += P_THREADS) {
        double s = 0.0;
        for (int wv = 0; wv < P_THREADS / 64; ++wv) s += rows[wv * nl + r];
        partial[(long long)r * gridDim.x + blockIdx.x] = s;
    }
}

template <bool LDS>
__global__ __launch_bounds__(P_THREADS) void pairmin_grad_kernel(PairArgs p, float scale, float* __restrict__ work, float* __restrict__ dx) {
    extern __shared__ __align__(16) float smem[];
    const int nl = p.hi - p.lo;
    const long long chunks = (p.n + P_THREADS - 1) / P_THREADS;
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const long long e = ch * P_THREADS + threadIdx.x;
        if (e >= p.n) continue;                                              // (no barrier below: every column is private to its thread)
        const long long stride = LDS ? P_THREADS : p.n, col = LDS ? threadIdx.x : e;
        float* vals = LDS ? smem : work;
        float* acc = LDS ? smem + (size_t)p.Bg * P_THREADS : dx;           // [nl] sums of signs; the global form accumulates in dx itself
        for (int a = 0; a < p.Bg; ++a) vals[(long long)a * stride + col] = p.x[(long long)a * p.n + e];
        for (int b = 0; b < nl; ++b) acc[(long long)b * stride + col] = 0.f;
        for (int r0 = 0; r0 < p.Bg; r0 += P_TILE) {
            float sd[P_TILE];
            int arg[P_TILE];
            walk_tile<true>(vals, stride, col, p.clamp01 != 0, p.Bg, r0, p.Bg, sd, arg);
#pragma unroll
            for (int k = 0; k < P_TILE; ++k) {
                const int r = r0 + k, a = arg[k];
                if (r >= p.Bg || a == r) continue;                           // the diagonal won: no gradient
                const float s = sgn(sd[k]);                                  // sign(I_r - I_a)
                if (r >= p.lo && r < p.hi) acc[(long long)(r - p.lo) * stride + col] += s;
                if (a >= p.lo && a < p.hi) acc[(long long)(a - p.lo) * stride + col] -= s;
            }
        }
        const float m = scale * (p.mask ? p.mask[e % p.hw] : 1.f);
        // outputs in groups of 8 rows, the loads of a group ahead of its stores (the compiler must assume that dx may alias init)
        const float* init = p.init ? p.init + e : nullptr;
        for (int b0 = 0; b0 < nl; b0 += 8) {
            float g[8], raw[8], i0[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int b = b0 + j < nl ? b0 + j : nl - 1;
                g[j] = acc[(long long)b * stride + col];
                raw[j] = vals[(long long)(b + p.lo) * stride + col];
                i0[j] = init ? init[(p.init_batch == 1 ? 0 : (long long)b) * p.n] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (b0 + j >= nl) break;
                if (init) g[j] -= p.w * sgn(rd(raw[j], p.clamp01 != 0) - i0[j]);
                if (p.clamp01 && !clamp_gate(raw[j])) g[j] = 0.f;
                dx[(long long)(b0 + j) * p.n + e] = m * g[j];
            }
        }
    }
}

bool fill_args(PairArgs& p, const float* x, int Bg, int C, int H, int W, int lo, int hi, int clamp01, const float* mask, const float* init,
               int init_batch, float w) {
    if (!x || Bg <= 0 || C <= 0 || H <= 0 || W <= 0 || lo < 0 || hi <= lo || hi > Bg) return false;
    if (init && init_batch != 1 && init_batch != hi - lo) return false;
    p.x = x, p.mask = mask, p.init = init;
    p.hw = (long long)H * W, p.n = p.hw * C;
    p.Bg = Bg, p.lo = lo, p.hi = hi, p.clamp01 = clamp01, p.init_batch = init_batch, p.w = w;
    return true;
}

unsigned grid_for(long long n) {
    const long long chunks = (n + P_THREADS - 1) / P_THREADS;
    return (unsigned)(chunks < P_MAX_BLOCKS ? chunks : P_MAX_BLOCKS);
}

}  // namespace

extern "C" int64_t esr_pairmin_blocks(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return ESR_E_ARG;
    return (int64_t)grid_for((long long)C * H * W);
}

extern "C" int64_t esr_pairmin_work_floats(int Bg, int C, int H, int W, int lo, int hi, int grad) {
    if (Bg <= 0 || C <= 0 || H <= 0 || W <= 0 || lo < 0 || hi <= lo || hi > Bg) return ESR_E_ARG;
    const size_t lds = grad ? ((size_t)Bg + (hi - lo)) * P_THREADS * sizeof(float)
                            : (size_t)Bg * P_THREADS * sizeof(float) + (size_t)(P_THREADS / 64) * (hi - lo) * sizeof(double);
    return lds <= P_LDS_LIMIT ? 0 : (int64_t)Bg * C * H * W;
}

extern "C" int esr_pairmin(const float* x, int Bg, int C, int H, int W, int lo, int hi, int clamp01, const float* mask, const float* init,
                           int init_batch, float w, float* work, double* partial, esr_stream_t stream) {
    PairArgs p;
    if (!partial || !fill_args(p, x, Bg, C, H, W, lo, hi, clamp01, mask, init, init_batch, w)) return ESR_E_ARG;
    const size_t rows = (size_t)(P_THREADS / 64) * (hi - lo) * sizeof(double);
    const size_t lds = (size_t)Bg * P_THREADS * sizeof(float) + rows;
    if (rows > P_LDS_LIMIT) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    if (lds <= P_LDS_LIMIT) {
        ESR_ALLOW_160K_LDS(pairmin_kernel<true>);
        hipLaunchKernelGGL(pairmin_kernel<true>, dim3(grid_for(p.n)), dim3(P_THREADS), lds, (hipStream_t)stream, p, (float*)nullptr, partial);
    } else {
        if (!work) return ESR_E_ARG;
        ESR_ALLOW_160K_LDS(pairmin_kernel<false>);
        hipLaunchKernelGGL(pairmin_kernel<false>, dim3(grid_for(p.n)), dim3(P_THREADS), rows, (hipStream_t)stream, p, work, partial);
    }
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_pairmin_grad(const float* x, int Bg, int C, int H, int W, int lo, int hi, int clamp01, const float* mask, const float* init,
                                int init_batch, float w, float scale, float* work, float* dx, esr_stream_t stream) {
    PairArgs p;
    if (!dx || !fill_args(p, x, Bg, C, H, W, lo, hi, clamp01, mask, init, init_batch, w)) return ESR_E_ARG;
    const size_t lds = ((size_t)Bg + (hi - lo)) * P_THREADS * sizeof(float);
    ESR_CLEAR_ERR();
    if (lds <= P_LDS_LIMIT) {
        ESR_ALLOW_160K_LDS(pairmin_grad_kernel<true>);
        hipLaunchKernelGGL(pairmin_grad_kernel<true>, dim3(grid_for(p.n)), dim3(P_THREADS), lds, (hipStream_t)stream, p, scale, (float*)nullptr, dx);
    } else {
        if (!work) return ESR_E_ARG;
        hipLaunchKernelGGL(pairmin_grad_kernel<false>, dim3(grid_for(p.n)), dim3(P_THREADS), 0, (hipStream_t)stream, p, scale, work, dx);
    }
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
