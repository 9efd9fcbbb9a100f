// The VGG feature extractor's glue between the conv launches (codes/models/modules/architecture.py:658-705, torchvision's VGG `features`):
// the input normalisation (x - mean) / std fused into the NCHW -> activation-layout pack, its adjoint fused into the gradient unpack, and the
// 2x2 stride-2 max pool with its backward.  The convolutions themselves (and their ReLU, act_slope = 0) are esr_conv3x3 launches.
// All four kernels are HBM-bound streaming kernels: one thread per 16-byte pixel vector (8 channels) of the destination.
#include "esr_common.h"

namespace {

// element e (0..7) of a 16-byte vector of 16-bit values
__device__ __forceinline__ uint32_t lane16(const uint4& v, int e) {
    const uint32_t w = (e >> 1) == 0 ? v.x : (e >> 1) == 1 ? v.y : (e >> 1) == 2 ? v.z : v.w;
    return (e & 1) ? (w >> 16) : (w & 0xFFFFu);
}
__device__ __forceinline__ float val16(uint32_t h, int fmt) { return fmt == ESR_FMT_F16 ? h2f(h) : bf2f(h); }
__device__ __forceinline__ uint4 pack8(const uint32_t (&e)[8]) {
    return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

// fp32 NCHW [B][C][h][w] -> act view (h x w interior, zero border), v = (x - mean[c]) / std[c] (mean / std NULL: v = x)
__global__ void pack_norm_kernel(const float* __restrict__ src, int C, int h, int w, const float* __restrict__ mean, const float* __restrict__ stdv,
                                 uint4* hi, uint4* lo, long long bs, long long cs, int ncg, int fmt, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int Wp = w + 2, Hp = h + 2;
    const int X = (int)(idx % Wp);
    long long t = idx / Wp;
    const int Y = (int)(t % Hp);
    t /= Hp;
    const int cg = (int)(t % ncg);
    const int b = (int)(t / ncg);
    const bool border = X == 0 || Y == 0 || X == Wp - 1 || Y == Hp - 1;
    uint32_t vh[8], vl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = cg * 8 + e;
        float v = 0.f;
        if (!border && ch < C) {
            v = src[(((long long)b * C + ch) * h + (Y - 1)) * w + (X - 1)];
            if (mean) v = (v - mean[ch]) / stdv[ch];
        }
        if (fmt == ESR_FMT_F16) { vh[e] = f2h(v); vl[e] = f2h(v - h2f(vh[e])); }
        else split_bf16(v, vh[e], vl[e]);
    }
    const long long o = b * bs + cg * cs + (long long)Y * Wp + X;
    hi[o] = pack8(vh);
    if (lo) lo[o] = pack8(vl);
}

// act-layout gradient (interior h x w) -> fp32 NCHW [B][C][h][w], divided by std[c] (std NULL: copied)
__global__ void unpack_grad_norm_kernel(DView g, int C, int h, int w, const float* __restrict__ stdv, float* __restrict__ dst, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per output element (b, c, y, x)
    if (idx >= total) return;
    const int x = (int)(idx % w);
    long long t = idx / w;
    const int y = (int)(t % h);
    t /= h;
    const int c = (int)(t % C);
    const int b = (int)(t / C);
    const long long o = b * g.bs + (c >> 3) * g.cs + (long long)(y + 1) * (w + 2) + (x + 1);
    float v = val16(lane16(g.hi[o], c & 7), g.fmt);
    if (g.lo) v += val16(lane16(g.lo[o], c & 7), g.fmt);
    dst[idx] = stdv ? v / stdv[c] : v;
}

// the window position (0..3, row-major) F.max_pool2d(2) takes for lane e: the first maximum of hi + lo, a NaN wins (and the last NaN is kept,
// as torch's `val > maxval || isnan(val)` update does)
__device__ __forceinline__ int window_argmax(const uint4 (&wh)[4], const uint4 (&wl)[4], bool has_lo, int fmt, int e) {
    float best = -__builtin_inff();
    int arg = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v = val16(lane16(wh[k], e), fmt);
        if (has_lo) v += val16(lane16(wl[k], e), fmt);
        if (v > best || __builtin_isnan(v)) { best = v; arg = k; }
    }
    return arg;
}

__device__ __forceinline__ void load_window(const DView& x, int Win, int b, int cg, int oy, int ox, uint4 (&wh)[4], uint4 (&wl)[4]) {
    const long long base = b * x.bs + cg * x.cs + (long long)(2 * oy + 1) * (Win + 2) + (2 * ox + 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long o = base + (long long)(k >> 1) * (Win + 2) + (k & 1);
        wh[k] = x.hi[o];
        wl[k] = x.lo ? x.lo[o] : make_uint4(0, 0, 0, 0);
    }
}

// y (Ho x Wo, Ho = floor(H / 2), Wo = floor(W / 2)) = max over each 2x2 window of x; the value at the argmax is copied bit for bit (hi and lo);
// the border of y is written as zeros
__global__ void maxpool_kernel(DView x, int Win, DView y, int Ho, int Wo, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int Wp = Wo + 2, Hp = Ho + 2;
    const int X = (int)(idx % Wp);
    long long t = idx / Wp;
    const int Y = (int)(t % Hp);
    t /= Hp;
    const int cg = (int)(t % y.ncg);
    const int b = (int)(t / y.ncg);
    const long long o = b * y.bs + cg * y.cs + (long long)Y * Wp + X;
    uint4* const yh = (uint4*)y.hi;
    uint4* const yl = (uint4*)y.lo;
    if (X == 0 || Y == 0 || X == Wp - 1 || Y == Hp - 1) {
        yh[o] = make_uint4(0, 0, 0, 0);
        if (yl) yl[o] = make_uint4(0, 0, 0, 0);
        return;
    }
    uint4 wh[4], wl[4];
    load_window(x, Win, b, cg, Y - 1, X - 1, wh, wl);
    uint32_t oh[8], ol[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = window_argmax(wh, wl, x.lo != nullptr, x.fmt, e);
        oh[e] = lane16(wh[k], e);
        ol[e] = lane16(wl[k], e);
    }
    yh[o] = pack8(oh);
    if (yl) yl[o] = pack8(ol);
}

// dx (H x W, zero border) = dy scattered to the argmax of every window of x (recomputed from x), zero elsewhere — including the last row /
// column of an odd size, which no window covers.  relu_mask: also zero where x <= 0 (x is the output of a ReLU: its backward, fused).
__global__ void maxpool_grad_kernel(DView x, DView dy, int Ho, int Wo, DView dx, int H, int W, int relu_mask, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int Wp = W + 2, Hp = H + 2;
    const int X = (int)(idx % Wp);
    long long t = idx / Wp;
    const int Y = (int)(t % Hp);
    t /= Hp;
    const int cg = (int)(t % dx.ncg);
    const int b = (int)(t / dx.ncg);
    const long long o = b * dx.bs + cg * dx.cs + (long long)Y * Wp + X;
    uint4* const gh = (uint4*)dx.hi;
    uint4* const gl = (uint4*)dx.lo;
    const int yy = Y - 1, xx = X - 1;
    if (yy < 0 || xx < 0 || yy >= 2 * Ho || xx >= 2 * Wo) {
        gh[o] = make_uint4(0, 0, 0, 0);
        if (gl) gl[o] = make_uint4(0, 0, 0, 0);
        return;
    }
    const int oy = yy >> 1, ox = xx >> 1, self = ((yy & 1) << 1) | (xx & 1);
    uint4 wh[4], wl[4];
    load_window(x, W, b, cg, oy, ox, wh, wl);
    const long long od = b * dy.bs + cg * dy.cs + (long long)(oy + 1) * (Wo + 2) + (ox + 1);
    const uint4 dh = dy.hi[od];
    const uint4 dl = dy.lo ? dy.lo[od] : make_uint4(0, 0, 0, 0);
    uint32_t oh[8], ol[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        bool pass = window_argmax(wh, wl, x.lo != nullptr, x.fmt, e) == self;
        if (relu_mask) {
            float v = val16(lane16(wh[self], e), x.fmt);
            if (x.lo) v += val16(lane16(wl[self], e), x.fmt);
            pass = pass && v > 0.f;
        }
        oh[e] = pass ? lane16(dh, e) : 0u;
        ol[e] = pass ? lane16(dl, e) : 0u;
    }
    gh[o] = pack8(oh);
    if (gl) gl[o] = pack8(ol);
}

inline unsigned blocks_of(long long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

extern "C" int esr_pack_nchw_norm(const float* src, int B, int C, int h, int w, const float* mean, const float* std, const esr_act_view* dst,
                                  esr_stream_t stream) {
    if (!src || !dst || !dst->hi || B <= 0 || C <= 0 || h <= 0 || w <= 0 || (!mean) != (!std)) return ESR_E_ARG;
    if (dst->H != h || dst->W != w || dst->ncg * 8 < C) return ESR_E_ARG;
    const long long total = (long long)B * dst->ncg * (h + 2) * (w + 2);
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(pack_norm_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, src, C, h, w, mean, std, (uint4*)dst->hi,
                       (uint4*)dst->lo, (long long)dst->batch_stride, (long long)dst->cg_stride, dst->ncg, dst->fmt, total);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_unpack_grad_nchw_norm(const esr_act_view* G, int B, int C, const float* std, float* dst, esr_stream_t stream) {
    if (!G || !G->hi || !dst || B <= 0 || C <= 0 || G->ncg * 8 < C || G->H <= 0 || G->W <= 0) return ESR_E_ARG;
    const long long total = (long long)B * C * G->H * G->W;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(unpack_grad_norm_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, to_dview(*G), C, G->H, G->W, std, dst, total);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_maxpool2x2(const esr_act_view* x, const esr_act_view* y, int B, esr_stream_t stream) {
    if (!x || !y || !x->hi || !y->hi || B <= 0 || x->fmt != y->fmt || (x->lo != nullptr) != (y->lo != nullptr)) return ESR_E_ARG;
    if (x->H < 2 || x->W < 2 || y->H != x->H / 2 || y->W != x->W / 2 || y->ncg <= 0 || y->ncg > x->ncg) return ESR_E_ARG;
    const long long total = (long long)B * y->ncg * (y->H + 2) * (y->W + 2);
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(maxpool_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, to_dview(*x), x->W, to_dview(*y), y->H, y->W, total);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_maxpool2x2_grad(const esr_act_view* x, const esr_act_view* dy, int relu_mask, const esr_act_view* dx, int B, esr_stream_t stream) {
    if (!x || !dy || !dx || !x->hi || !dy->hi || !dx->hi || B <= 0) return ESR_E_ARG;
    if (dy->fmt != dx->fmt || (dy->lo != nullptr) != (dx->lo != nullptr)) return ESR_E_ARG;
    if (x->H < 2 || x->W < 2 || dx->H != x->H || dx->W != x->W || dy->H != x->H / 2 || dy->W != x->W / 2) return ESR_E_ARG;
    if (dx->ncg <= 0 || dx->ncg > x->ncg || dx->ncg > dy->ncg) return ESR_E_ARG;
    const long long total = (long long)B * dx->ncg * (dx->H + 2) * (dx->W + 2);
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(maxpool_grad_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, to_dview(*x), to_dview(*dy), dy->H, dy->W,
                       to_dview(*dx), dx->H, dx->W, relu_mask, total);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
