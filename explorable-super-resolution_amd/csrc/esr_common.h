// Shared device helpers for the gfx950 kernels of libesr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/esr_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// float -> bf16 bits, round to nearest even (finite inputs; NaN stays NaN-ish, never produced on this path)
__device__ __forceinline__ uint32_t f2bf(float x) {
    uint32_t u = __float_as_uint(x);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ float bf2f(uint32_t h) { return __uint_as_float(h << 16); }

// split x into hi = bf16(x), lo = bf16(x - hi); hi + lo carries ~16 mantissa bits of x
__device__ __forceinline__ void split_bf16(float x, uint32_t& hi, uint32_t& lo) {
    hi = f2bf(x);
    lo = f2bf(x - bf2f(hi));
}

// fp16 element <-> float (round to nearest even)
__device__ __forceinline__ uint32_t f2h(float x) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)x); }
__device__ __forceinline__ float h2f(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)h); }
// 16-bit element of format FMT (0 bf16, 1 f16) <-> float
template <int FMT> __device__ __forceinline__ float e2f(uint32_t e) { return FMT ? h2f(e) : bf2f(e); }
template <int FMT> __device__ __forceinline__ uint32_t f2e(float x) { return FMT ? f2h(x) : f2bf(x); }

// device-side mirror of esr_act_view (strides in 16-byte vectors)
struct DView {
    const uint4* hi;
    const uint4* lo;
    long long bs, cs;
    int ncg;
    int fmt;
};

static inline DView to_dview(const esr_act_view& v) {
    DView d;
    d.hi = (const uint4*)v.hi;
    d.lo = (const uint4*)v.lo;
    d.bs = v.batch_stride;
    d.cs = v.cg_stride;
    d.ncg = v.hi ? v.ncg : 0;
    d.fmt = v.fmt;
    return d;
}

// ---- The activation layout, for every kernel that is not an MFMA kernel (those are templated on FMT and keep their own code) -------------
// [planes][B][CG][H+2][W+2][8] 16-bit elements: a `hi` plane and an optional `lo` plane of residuals (value = hi + lo), both in format
// `fmt` (ESR_FMT_BF16 / ESR_FMT_F16, uniform per view), one 16-byte vector per (image, channel group, pixel), a one-pixel zero border.
// The accessors take raw plane pointers, strides and fmt, so they serve DView, the critic's view and kernels that receive the fields one by one.

// offset (in vectors) of position (Y, X) of the padded (H+2) x (W+2) frame, and of interior pixel (y, x), of group cg of image b
__device__ __forceinline__ long long act_off_frame(long long bs, long long cs, int W, int b, int cg, int Y, int X) {
    return b * bs + cg * cs + (long long)Y * (W + 2) + X;
}
__device__ __forceinline__ long long act_off(long long bs, long long cs, int W, int b, int cg, int y, int x) {
    return act_off_frame(bs, cs, W, b, cg, y + 1, x + 1);
}

// flat thread index -> (i0, i1, i2, i3), i3 fastest, over a box [..][n1][n2][n3]
struct Idx4 { int i0, i1, i2, i3; };
__device__ __forceinline__ Idx4 split_index(long long idx, int n1, int n2, int n3) {
    Idx4 p;
    p.i3 = (int)(idx % n3);
    long long t = idx / n3;
    p.i2 = (int)(t % n2);
    t /= n2;
    p.i1 = (int)(t % n1);
    p.i0 = (int)(t / n1);
    return p;
}
// the same as (b, cg, y, x) over ncg groups of H x W positions per image (pass H+2, W+2 to walk the padded frame)
struct ActPos { int b, cg, y, x; };
__device__ __forceinline__ ActPos act_pos(long long idx, int ncg, int H, int W) {
    const Idx4 p = split_index(idx, ncg, H, W);
    return ActPos{p.i0, p.i1, p.i2, p.i3};
}
__device__ __forceinline__ bool frame_border(int Y, int X, int H, int W) { return X == 0 || Y == 0 || X == W + 1 || Y == H + 1; }

// element e (0..7) of a 16-byte vector of 16-bit values, and the vector of eight such values
__device__ __forceinline__ uint32_t elem16(const uint4& v, int e) {
    const uint32_t w = (e >> 1) == 0 ? v.x : (e >> 1) == 1 ? v.y : (e >> 1) == 2 ? v.z : v.w;
    return (e & 1) ? (w >> 16) : (w & 0xFFFFu);
}
__device__ __forceinline__ uint4 pack16x8(const uint32_t (&e)[8]) {
    return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

// The raw vectors of one pixel (lo: zeros when the view has no lo plane) and their decoding for a run-time fmt, as two steps: a kernel may
// issue the loads of several pixels before it decodes the first.  A value is dec(hi) + dec(lo), in this order; an absent lo plane counts as
// +0 (so a stored -0 decodes to +0).  decode1 is one element of the pixel, decode8 all eight, load8 the two steps composed.
struct Raw8 { uint4 h, l; };
__device__ __forceinline__ Raw8 load_raw8(const uint4* hi, const uint4* lo, long long o) {
    Raw8 r;
    r.h = hi[o];
    r.l = lo ? lo[o] : make_uint4(0, 0, 0, 0);
    return r;
}
__device__ __forceinline__ float decode1(const Raw8& r, bool has_lo, int fmt, int e) {
    const uint32_t hb = elem16(r.h, e), lb = elem16(r.l, e);
    return fmt == ESR_FMT_F16 ? h2f(hb) + (has_lo ? h2f(lb) : 0.f) : bf2f(hb) + (has_lo ? bf2f(lb) : 0.f);
}
__device__ __forceinline__ void decode8(const Raw8& r, bool has_lo, int fmt, float (&f)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = decode1(r, has_lo, fmt, e);
}
__device__ __forceinline__ void load8(const uint4* hi, const uint4* lo, long long o, int fmt, float (&f)[8]) {
    decode8(load_raw8(hi, lo, o), lo != nullptr, fmt, f);
}

// Stores take writable planes.  DView mirrors read and written views alike, so its pointers are const: a kernel that writes through one
// says so with mut() at the call.
__device__ __forceinline__ uint4* mut(const uint4* plane) { return const_cast<uint4*>(plane); }
__device__ __forceinline__ void store_raw8(uint4* hi, uint4* lo, long long o, const Raw8& r) {
    hi[o] = r.h;
    if (lo) lo[o] = r.l;
}
// eight floats -> hi = fmt(v) and the residual lo = fmt(v - hi), as vectors.  The encoder is eight wide on purpose: with the format branch
// written once around the unrolled loop the compiler emits one uniform branch per pixel, not one per element.
__device__ __forceinline__ Raw8 encode8(const float (&f)[8], int fmt) {
    uint32_t vh[8], vl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (fmt == ESR_FMT_F16) { vh[e] = f2h(f[e]); vl[e] = f2h(f[e] - h2f(vh[e])); }
        else split_bf16(f[e], vh[e], vl[e]);
    }
    return Raw8{pack16x8(vh), pack16x8(vl)};
}
__device__ __forceinline__ void store8(uint4* hi, uint4* lo, long long o, const float (&f)[8], int fmt) {
    store_raw8(hi, lo, o, encode8(f, fmt));
}

// ---- scalar helpers of the image-space kernels
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float clamp_unit(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }      // torch's |.|' = 0 at 0
// mean over the C channels of the [0, 1]-clamped image at pixel offset `off` (planes `plane` apart)
__device__ __forceinline__ float gray(const float* __restrict__ img, int C, long long plane, long long off) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += clamp_unit(img[c * plane + off]);
    return s / (float)C;
}

// hipGetLastError() is sticky-until-read and shared with the host framework: drop whatever an earlier, unrelated call left
// behind before launching, so that ESR_CHECK_LAUNCH reports only our own launch
#define ESR_CLEAR_ERR() (void)hipGetLastError()
#define ESR_CHECK_LAUNCH()                                   \
    do {                                                     \
        hipError_t e__ = hipGetLastError();                  \
        if (e__ != hipSuccess) return ESR_E_LAUNCH;          \
    } while (0)

// Raise a kernel's dynamic-LDS limit to the full 160 KiB once per (kernel, device): the attribute is per device, and one process may
// drive several (host threads under nn.DataParallel-style use).  `mask` is a function-local static of the caller.
#define ESR_ALLOW_160K_LDS(kernel_ptr)                                                                                      \
    do {                                                                                                                    \
        static unsigned long long mask__ = 0;   /* benign race: setting the attribute twice is harmless */                  \
        int dev__ = 0;                                                                                                      \
        (void)hipGetDevice(&dev__);                                                                                         \
        if (!(mask__ >> (dev__ & 63) & 1ull)) {                                                                             \
            (void)hipFuncSetAttribute((const void*)(kernel_ptr), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);   \
            mask__ |= 1ull << (dev__ & 63);                                                                                 \
        }                                                                                                                   \
    } while (0)
