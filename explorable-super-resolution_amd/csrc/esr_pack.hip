// Layout conversion at the module boundary: fp32 NCHW <-> the channel-group activation layout of the conv kernels
// ([B][CG][H+2][W+2][8] bf16 hi/lo planes with a zero border), with the CEM eval-mode replicate padding
// (codes/CEM/CEMnet.py:286-295) and the latent bilinear /sf of RRDBNet.forward (codes/models/modules/architecture.py:284)
// fused into the read.  HBM-bound streaming kernels: one 16-byte vector store per thread, coalesced along W.
// The layout's arithmetic (offsets, index decomposition, encode / decode of a pixel vector) is esr_common.h's.
#include "esr_common.h"

namespace {

__global__ void pack_nchw_kernel(const float* __restrict__ src, long long sbs, int C, int h, int w, int c0, int nc, int pad, int down, uint4* hi,
                                 uint4* lo, long long bs, long long cs, int ncg, int Hd, int Wd, int fmt, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const ActPos q = act_pos(idx, ncg, Hd + 2, Wd + 2);   // over the padded frame
    const int b = q.b, cg = q.cg, Y = q.y, X = q.x;
    const bool border = frame_border(Y, X, Hd, Wd);
    float v8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = cg * 8 + e;
        float v = 0.f;
        if (!border && ch < nc) {
            const float* p = src + b * sbs + ((long long)(c0 + ch) * h) * w;
            const int y = Y - 1, x = X - 1;
            if (down == 1) {
                v = p[(long long)clampi(y - pad, 0, h - 1) * w + clampi(x - pad, 0, w - 1)];
            } else {
                // F.interpolate(bilinear, align_corners=False, scale_factor=1/down) on the replicate-padded frame
                const int hp = h + 2 * pad, wp = w + 2 * pad;
                float sy = fmaxf((y + 0.5f) * (float)down - 0.5f, 0.f), sx = fmaxf((x + 0.5f) * (float)down - 0.5f, 0.f);
                const int y0 = (int)sy, x0 = (int)sx;
                const int y1 = y0 + (y0 < hp - 1 ? 1 : 0), x1 = x0 + (x0 < wp - 1 ? 1 : 0);
                const float ly = sy - (float)y0, lx = sx - (float)x0;
                const long long r0 = (long long)clampi(y0 - pad, 0, h - 1) * w, r1 = (long long)clampi(y1 - pad, 0, h - 1) * w;
                const int q0 = clampi(x0 - pad, 0, w - 1), q1 = clampi(x1 - pad, 0, w - 1);
                v = (1.f - ly) * ((1.f - lx) * p[r0 + q0] + lx * p[r0 + q1]) + ly * ((1.f - lx) * p[r1 + q0] + lx * p[r1 + q1]);
            }
        }
        v8[e] = v;
    }
    store8(hi, lo, act_off_frame(bs, cs, Wd, b, cg, Y, X), v8, fmt);
}

__global__ void unpack_nchw_kernel(const uint4* __restrict__ hi, const uint4* __restrict__ lo, long long bs, long long cs, int H, int W,
                                   int nc, float* __restrict__ dst, int fmt, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (b, cg, y, x)
    if (idx >= total) return;
    const ActPos q = act_pos(idx, (nc + 7) / 8, H, W);
    const int b = q.b, cg = q.cg, y = q.y, x = q.x;
    float v8[8];
    load8(hi, lo, act_off(bs, cs, W, b, cg, y, x), fmt, v8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = cg * 8 + e;
        if (ch >= nc) break;
        dst[((long long)(b * nc + ch) * H + y) * W + x] = v8[e];
    }
}

__global__ void zero_kernel(uint4* p, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = i; k < n; k += stride) p[k] = make_uint4(0, 0, 0, 0);
}

}  // namespace

extern "C" int esr_pack_nchw(const float* src, int64_t src_batch_stride, int B, int C, int h, int w, int c0, int nc, int pad, int down, const esr_act_view* dst,
                             esr_stream_t stream) {
    if (!src || !dst || !dst->hi || B <= 0 || nc <= 0 || c0 < 0 || c0 + nc > C || pad < 0 || down < 1) return ESR_E_ARG;
    if (h < 1 || w < 1) return ESR_E_ARG;   // nothing to replicate: the clamp would read src[-1]
    if ((h + 2 * pad) % down || (w + 2 * pad) % down) return ESR_E_ARG;
    const int Hd = (h + 2 * pad) / down, Wd = (w + 2 * pad) / down;
    if (dst->H != Hd || dst->W != Wd || dst->ncg * 8 < nc) return ESR_E_ARG;
    const long long total = (long long)B * dst->ncg * (Hd + 2) * (Wd + 2);
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(pack_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                       (long long)(src_batch_stride ? src_batch_stride : (int64_t)C * h * w), C, h, w, c0, nc, pad,
                       down, (uint4*)dst->hi, (uint4*)dst->lo, (long long)dst->batch_stride, (long long)dst->cg_stride, dst->ncg, Hd, Wd, dst->fmt, total);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_unpack_nchw(const esr_act_view* src, int B, int nc, float* dst, esr_stream_t stream) {
    if (!src || !src->hi || !dst || B <= 0 || nc <= 0 || src->ncg * 8 < nc) return ESR_E_ARG;
    if (src->H < 1 || src->W < 1) return ESR_E_ARG;   // an empty grid is a launch error, not a no-op
    const long long total = (long long)B * ((nc + 7) / 8) * src->H * src->W;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(unpack_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)src->hi,
                       (const uint4*)src->lo, (long long)src->batch_stride, (long long)src->cg_stride, src->H, src->W, nc, dst, src->fmt, total);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_zero(void* p, int64_t n16, esr_stream_t stream) {
    if (!p || n16 < 0) return ESR_E_ARG;
    if (n16 == 0) return ESR_OK;
    long long blocks = (n16 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)p, (long long)n16);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_version(void) { return 101; }
