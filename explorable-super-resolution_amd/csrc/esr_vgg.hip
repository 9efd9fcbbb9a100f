// The VGG feature extractor's glue between the conv launches (codes/models/modules/architecture.py:658-705, torchvision's VGG `features`):
// the input normalisation (x - mean) / std fused into the NCHW -> activation-layout pack, its adjoint fused into the gradient unpack, and the
// 2x2 stride-2 max pool with its backward.  The convolutions themselves (and their ReLU, act_slope = 0) are esr_conv3x3 launches.
// All four kernels are HBM-bound streaming kernels: one thread per 16-byte pixel vector (8 channels) of the destination; they read and
// write the layout through the accessors of esr_common.h.
#include "esr_common.h"

namespace {

// fp32 NCHW [B][C][h][w] -> act view (h x w interior, zero border), v = (x - mean[c]) / std[c] (mean / std NULL: v = x)
__global__ void pack_norm_kernel(const float* __restrict__ src, int C, int h, int w, const float* __restrict__ mean, const float* __restrict__ stdv,
                                 uint4* hi, uint4* lo, long long bs, long long cs, int ncg, int fmt, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const ActPos q = act_pos(idx, ncg, h + 2, w + 2);   // over the padded frame
    const int b = q.b, cg = q.cg, Y = q.y, X = q.x;
    const bool border = frame_border(Y, X, h, w);
    float v8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = cg * 8 + e;
        float v = 0.f;
        if (!border && ch < C) {
            v = src[(((long long)b * C + ch) * h + (Y - 1)) * w + (X - 1)];
            if (mean) v = (v - mean[ch]) / stdv[ch];
        }
        v8[e] = v;
    }
    store8(hi, lo, act_off_frame(bs, cs, w, b, cg, Y, X), v8, fmt);
}

// act-layout gradient (interior h x w) -> fp32 NCHW [B][C][h][w], divided by std[c] (std NULL: copied)
__global__ void unpack_grad_norm_kernel(DView g, int C, int h, int w, const float* __restrict__ stdv, float* __restrict__ dst, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per output element (b, c, y, x)
    if (idx >= total) return;
    const Idx4 q = split_index(idx, C, h, w);
    const int b = q.i0, c = q.i1, y = q.i2, x = q.i3;
    const float v = decode1(load_raw8(g.hi, g.lo, act_off(g.bs, g.cs, w, b, c >> 3, y, x)), g.lo != nullptr, g.fmt, c & 7);
    dst[idx] = stdv ? v / stdv[c] : v;
}

// the window position (0..3, row-major) F.max_pool2d(2) takes for lane e: the first maximum of hi + lo, a NaN wins (and the last NaN is kept,
// as torch's `val > maxval || isnan(val)` update does)
__device__ __forceinline__ int window_argmax(const uint4 (&wh)[4], const uint4 (&wl)[4], bool has_lo, int fmt, int e) {
    float best = -__builtin_inff();
    int arg = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float v = decode1(Raw8{wh[k], wl[k]}, has_lo, fmt, e);
        if (v > best || __builtin_isnan(v)) { best = v; arg = k; }
    }
    return arg;
}

__device__ __forceinline__ void load_window(const DView& x, int Win, int b, int cg, int oy, int ox, uint4 (&wh)[4], uint4 (&wl)[4]) {
    const long long base = act_off(x.bs, x.cs, Win, b, cg, 2 * oy, 2 * ox);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Raw8 r = load_raw8(x.hi, x.lo, base + (long long)(k >> 1) * (Win + 2) + (k & 1));
        wh[k] = r.h;
        wl[k] = r.l;
    }
}

// y (Ho x Wo, Ho = floor(H / 2), Wo = floor(W / 2)) = max over each 2x2 window of x; the value at the argmax is copied bit for bit (hi and lo);
// the border of y is written as zeros
__global__ void maxpool_kernel(DView x, int Win, DView y, int Ho, int Wo, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const ActPos q = act_pos(idx, y.ncg, Ho + 2, Wo + 2);   // over y's padded frame
    const int b = q.b, cg = q.cg, Y = q.y, X = q.x;
    const long long o = act_off_frame(y.bs, y.cs, Wo, b, cg, Y, X);
    if (frame_border(Y, X, Ho, Wo)) {
        store_raw8(mut(y.hi), mut(y.lo), o, Raw8{});
        return;
    }
    uint4 wh[4], wl[4];
    load_window(x, Win, b, cg, Y - 1, X - 1, wh, wl);
    uint32_t oh[8], ol[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = window_argmax(wh, wl, x.lo != nullptr, x.fmt, e);
        oh[e] = elem16(wh[k], e);
        ol[e] = elem16(wl[k], e);
    }
    store_raw8(mut(y.hi), mut(y.lo), o, Raw8{pack16x8(oh), pack16x8(ol)});
}

// dx (H x W, zero border) = dy scattered to the argmax of every window of x (recomputed from x), zero elsewhere — including the last row /
// column of an odd size, which no window covers.  relu_mask: also zero where x <= 0 (x is the output of a ReLU: its backward, fused).
__global__ void maxpool_grad_kernel(DView x, DView dy, int Ho, int Wo, DView dx, int H, int W, int relu_mask, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const ActPos q = act_pos(idx, dx.ncg, H + 2, W + 2);   // over dx's padded frame
    const int b = q.b, cg = q.cg, Y = q.y, X = q.x;
    const long long o = act_off_frame(dx.bs, dx.cs, W, b, cg, Y, X);
    const int yy = Y - 1, xx = X - 1;
    if (yy < 0 || xx < 0 || yy >= 2 * Ho || xx >= 2 * Wo) {
        store_raw8(mut(dx.hi), mut(dx.lo), o, Raw8{});
        return;
    }
    const int oy = yy >> 1, ox = xx >> 1, self = ((yy & 1) << 1) | (xx & 1);
    uint4 wh[4], wl[4];
    load_window(x, W, b, cg, oy, ox, wh, wl);
    const Raw8 d = load_raw8(dy.hi, dy.lo, act_off(dy.bs, dy.cs, Wo, b, cg, oy, ox));
    uint32_t oh[8], ol[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        bool pass = window_argmax(wh, wl, x.lo != nullptr, x.fmt, e) == self;
        if (relu_mask) pass = pass && decode1(Raw8{wh[self], wl[self]}, x.lo != nullptr, x.fmt, e) > 0.f;
        oh[e] = pass ? elem16(d.h, e) : 0u;
        ol[e] = pass ? elem16(d.l, e) : 0u;
    }
    store_raw8(mut(dx.hi), mut(dx.lo), o, Raw8{pack16x8(oh), pack16x8(ol)});
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
