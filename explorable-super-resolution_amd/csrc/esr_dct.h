// Shared by the block-DCT kernels of the JPEG consistency layer (esr_jpeg.hip: 8-point, esr_jpeg16.hip: 16-point, esr_jpeg_edit.hip: the editing
// tools on both): the cosine tables and the 16-point one-dimensional transforms, and the coefficient side of a workgroup tile.  Coefficient planes are contiguous along w (blocks per image row); a thread moves four consecutive w positions of one plane,
// as one 16-byte access when `vec` (w % 4 == 0 and every pointer of the call 16-byte aligned: coef_vec) and element by element otherwise.
// The generator's sigmoid tail and its backward are fused here.  `o` is the element offset in coef, `oy` the one in y / dy / coef_out, which
// the 16-point kernels index as a tensor of another channel count; the 8-point kernels pass the same offset twice.
#pragma once
#include <math.h>

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

// ---- the transforms: the cosine tables (computed in double on the host, once; a by-value kernel argument, so that with the loops unrolled
// every cosine is a scalar operand) and the 16-point one-dimensional transforms
struct DctTab {
    float c[64];  // c[8k + n] = a(k) cos((2n + 1) k pi / 16), a(0) = sqrt(1/8), a(k > 0) = 1/2: the orthonormal DCT-II matrix
};

const DctTab& dct_tab() {
    static const DctTab tab = [] {
        DctTab t;
        for (int k = 0; k < 8; ++k)
            for (int n = 0; n < 8; ++n)
                t.c[8 * k + n] = (float)((k == 0 ? sqrt(0.125) : 0.5) * cos((2 * n + 1) * k * M_PI / 16.0));
        return t;
    }();
    return tab;
}

struct Dct16Tab {
    float c[128];  // c[8k + n] = a(k) cos((2n + 1) k pi / 32), n < 8;  a(0) = 1/4, a(k > 0) = sqrt(1/8)
};

const Dct16Tab& dct16_tab() {
    static const Dct16Tab tab = [] {
        Dct16Tab t;
        for (int k = 0; k < 16; ++k)
            for (int n = 0; n < 8; ++n) t.c[8 * k + n] = (float)((k == 0 ? 0.25 : sqrt(0.125)) * cos((2 * n + 1) * k * M_PI / 32.0));
        return t;
    }();
    return tab;
}

// out[k] = sum_n c(k, n) x[n], k < K, by the even/odd split
template <int K>
__device__ __forceinline__ void dct16(const Dct16Tab& tab, const float (&x)[16], float (&out)[16]) {
    float e[8], o[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        e[n] = x[n] + x[15 - n];
        o[n] = x[n] - x[15 - n];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
#pragma unroll
        for (int n = 0; n < 8; ++n) s = fmaf(tab.c[8 * k + n], (k & 1) ? o[n] : e[n], s);
        out[k] = s;
    }
}

// x[n] = sum_{k < K} c(k, n) in[k], n < 16
template <int K>
__device__ __forceinline__ void idct16(const Dct16Tab& tab, const float (&in)[16], float (&x)[16]) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        float e = 0.f, o = 0.f;
#pragma unroll
        for (int k = 0; k < K; k += 2) {
            e = fmaf(tab.c[8 * k + n], in[k], e);
            o = fmaf(tab.c[8 * (k + 1) + n], in[k + 1], o);
        }
        x[n] = e + o;
        x[15 - n] = e - o;
    }
}

// ---- host side of the entry points
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the 16-byte form of the coefficient side: rows of whole float4s, and every coefficient-side pointer of the call (null: not used) aligned
inline int coef_vec(int w, const void* a, const void* b = nullptr, const void* c = nullptr) {
    return (w % 4 == 0 && al16(a) && al16(b) && al16(c)) ? 1 : 0;
}
inline bool dims_positive(int B, int h, int w) { return B > 0 && h > 0 && w > 0; }
// grid z = image x plane, grid y = block row
inline bool grid_fits(int B, int planes, int h) { return (long long)B * planes <= 65535 && h <= 65535; }

}  // namespace
