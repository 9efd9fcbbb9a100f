// Shared by the block-DCT kernels of the JPEG consistency layer (esr_jpeg.hip: 8-point, esr_jpeg16.hip: 16-point): the coefficient side of a
// workgroup tile.  Coefficient planes are contiguous along w (blocks per image row); a thread moves four consecutive w positions of one plane,
// as one 16-byte access when `vec` (w % 4 == 0 and every pointer of the call 16-byte aligned: coef_vec) and element by element otherwise.
// The generator's sigmoid tail and its backward are fused here.  `o` is the element offset in coef, `oy` the one in y / dy / coef_out, which
// the 16-point kernels index as a tensor of another channel count; the 8-point kernels pass the same offset twice.
#pragma once
#include "esr_common.h"

namespace {

__device__ __forceinline__ float sigmoidf(float y) { return 1.f / (1.f + expf(-y)); }

// c = coef [+ sigmoid(y) - 0.5] at four w positions, the first n (> 0) of them inside the row and the rest 0; coef_out (optional) receives c.
// Returns c (/ or *) *qp.
__device__ __forceinline__ float4 coef_load4(const float* __restrict__ coef, const float* __restrict__ y, float* __restrict__ coef_out,
                                             long long o, long long oy, int vec, int n, const float* __restrict__ qp, int divide) {
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        const float4 v = *(const float4*)(coef + o);
        e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
        if (y) {
            const float4 yy = *(const float4*)(y + oy);
            e[0] += sigmoidf(yy.x) - 0.5f; e[1] += sigmoidf(yy.y) - 0.5f; e[2] += sigmoidf(yy.z) - 0.5f; e[3] += sigmoidf(yy.w) - 0.5f;
        }
        if (coef_out) *(float4*)(coef_out + oy) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
        for (int k = 0; k < 4 && k < n; ++k) {
            e[k] = coef[o + k];
            if (y) e[k] += sigmoidf(y[oy + k]) - 0.5f;
            if (coef_out) coef_out[oy + k] = e[k];
        }
    }
    const float q = *qp;
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = divide ? e[k] / q : e[k] * q;
    return make_float4(e[0], e[1], e[2], e[3]);
}

// the first n (> 0) of four w positions of v to coef (optional), and dy = v * s (1 - s), s = sigmoid(y), to dy (optional, with y)
__device__ __forceinline__ void coef_store4(const float4 v, float* __restrict__ coef, const float* __restrict__ y, float* __restrict__ dy,
                                            long long o, long long oy, int vec, int n) {
    if (vec) {
        if (coef) *(float4*)(coef + o) = v;
        if (dy) {
            const float4 yy = *(const float4*)(y + oy);
            const float s0 = sigmoidf(yy.x), s1 = sigmoidf(yy.y), s2 = sigmoidf(yy.z), s3 = sigmoidf(yy.w);
            *(float4*)(dy + oy) = make_float4(v.x * (s0 * (1.f - s0)), v.y * (s1 * (1.f - s1)), v.z * (s2 * (1.f - s2)), v.w * (s3 * (1.f - s3)));
        }
    } else {
        const float e[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < 4 && k < n; ++k) {
            if (coef) coef[o + k] = e[k];
            if (dy) {
                const float s = sigmoidf(y[oy + k]);
                dy[oy + k] = e[k] * (s * (1.f - s));
            }
        }
    }
}

// ---- host side of the eight entry points
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the 16-byte form of the coefficient side: rows of whole float4s, and every coefficient-side pointer of the call (null: not used) aligned
inline int coef_vec(int w, const void* a, const void* b = nullptr, const void* c = nullptr) {
    return (w % 4 == 0 && al16(a) && al16(b) && al16(c)) ? 1 : 0;
}
inline bool dims_positive(int B, int h, int w) { return B > 0 && h > 0 && w > 0; }
// grid z = image x plane, grid y = block row
inline bool grid_fits(int B, int planes, int h) { return (long long)B * planes <= 65535 && h <= 65535; }

}  // namespace
