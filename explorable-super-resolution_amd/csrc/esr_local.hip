// Local-STD and periodicity Z objectives (reference codes/Z_optimization.py:391-398, 459-509, 616-627, 799-815): the kernels behind the
// GUI's "increase / decrease local variance", "decrease TV" and "impose periodicity" tools.
//
// Patch STD.  For every 7 x 7 window whose top-left corner is selected in a uint8 corner map [H-6][W-6] (the windows inside the opened image
// mask; esr_hip/local.py builds the map), of the gray image v = mean_c clamp(x_c, 0, 1):
//     mean[p] = (1/49) sum v,   S[p] = sqrt( (1/48) sum (v - mean)^2 )       (torch.std, unbiased)
// The reference gathers the 49 x P values with torch.sparse.mm against a (49 P) x (H W) matrix per image; here a workgroup reads a 22 x 70
// tile of v into LDS (clamp and channel mean fused into the read, 1.5x read amplification) and every thread evaluates the windows of a few
// corners from LDS, two passes over the 49 values shifted by the window's first value: a flat window gives S = 0 exactly.
// Its gradient: with a[p] = dS[p] / (48 S[p]) (0 where S = 0 or the corner is unselected),
//     dv(y, x) = sum over the corners whose window covers (y, x) of a[p] (v(y, x) - mean[p])
// (the v Box7^T(a) - Box7^T(a mean) of the adjoint, evaluated per term so that nearly flat windows do not cancel), dx_c = dv / C [0 <= x_c <= 1].
// A workgroup owns a 16 x 64 pixel tile and stages a and mean of the 22 x 70 corners covering it in LDS: no atomics, bit-reproducible.
// The tiling of both directions is Patch7 of csrc/esr_image.h (shared with csrc/esr_patchmag.hip); the kernels here hold the arithmetic only.
//
// Shifted L1 (periodicity).  For one period point and its two signs s = +, -: separable bilinear samplers (grid_sample, zero padding) given as
// per-output-column taps (base_x[s][j], frac_x[s][j]) and per-output-row taps (base_y[s][i], frac_y[s][i]), weights (1 - frac, frac) on
// (base, base + 1).  Per image
//     sum_{c,i,j} M(i,j) |GS+(I)(c,i,j) - GS-(I)(c,i,j)|,   M = GS+(mask) GS-(mask),   I = clamp(x, 0, 1)
// as one double per (image, output row); the caller sums the rows and divides by C ny nx.  The backward forms G = g_b M sign(GS+ - GS-) on the
// output grid, then the adjoint Wy+^T G Wx+ - Wy-^T G Wx- in gather form: every source pixel walks the output rows / columns whose taps
// touch it, from per-source contributor ranges built by the caller (the samplers are monotone, so each range is contiguous).  No atomics.
#include "esr_image.h"

namespace {

using PT = Patch7;
constexpr int LP = PT::SIDE;                 // patch side (the reference's PATCH_SIZE_4_STD)
constexpr int L_THREADS = PT::NT;

__global__ __launch_bounds__(L_THREADS) void patch_std_kernel(const float* __restrict__ x, int C, int H, int W, const uint8_t* __restrict__ corners,
                                                                float* __restrict__ S, float* __restrict__ M) {
    __shared__ float v[PT::SY][PT::SX];
    PT::load_gray(v, x, C, H, W);
    const int b = blockIdx.z, Hc = H - LP + 1, Wc = W - LP + 1;
    PT::for_corners(H, W, [&](int cy, int cx, int ty, int tx) {
        const long long o = ((long long)b * Hc + cy) * Wc + cx;
        float s = 0.f, m = 0.f;
        if (corners[(long long)cy * Wc + cx]) {
            const float k = v[ty][tx];
            float s1 = 0.f;
#pragma unroll
            for (int dy = 0; dy < LP; ++dy)
#pragma unroll
                for (int dx = 0; dx < LP; ++dx) s1 += v[ty + dy][tx + dx] - k;
            const float md = s1 * (1.f / (LP * LP));
            float s2 = 0.f;
#pragma unroll
            for (int dy = 0; dy < LP; ++dy)
#pragma unroll
                for (int dx = 0; dx < LP; ++dx) {
                    const float d = v[ty + dy][tx + dx] - k - md;
                    s2 += d * d;
                }
            s = sqrtf(s2 / (float)(LP * LP - 1));
            m = k + md;
        }
        S[o] = s;
        M[o] = m;
    });
}

__global__ __launch_bounds__(L_THREADS) void patch_std_grad_kernel(const float* __restrict__ x, int C, int H, int W, const uint8_t* __restrict__ corners,
                                                                     const float* __restrict__ S, const float* __restrict__ M, const float* __restrict__ dS,
                                                                     float* __restrict__ dx, int accumulate) {
    __shared__ float a[PT::SY][PT::SX], m[PT::SY][PT::SX];
    const int b = blockIdx.z, Hc = H - LP + 1, Wc = W - LP + 1;
    const long long plane = (long long)H * W;
    PT::stage_corners(H, W, [&](int ty, int tx, int cy, int cx, bool inside) {
        float av = 0.f, mv = 0.f;
        if (inside && corners[(long long)cy * Wc + cx]) {
            const long long o = ((long long)b * Hc + cy) * Wc + cx;
            const float s = S[o];
            if (s > 0.f) {
                av = dS[o] / ((float)(LP * LP - 1) * s);
                mv = M[o];
            }
        }
        a[ty][tx] = av;
        m[ty][tx] = mv;
    });
    const float* img = x + (long long)b * C * plane;
    float* out = dx + (long long)b * C * plane;
    PT::for_pixels(H, W, [&](int y, int xx, int ty, int tx) {
        const long long off = (long long)y * W + xx;
        const float v = gray(img, C, plane, off);
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < LP; ++dy)
#pragma unroll
            for (int dxx = 0; dxx < LP; ++dxx) acc += a[ty + dy][tx + dxx] * (v - m[ty + dy][tx + dxx]);
        gated_store_pixel(out, img, C, plane, off, acc / (float)C, accumulate);
    });
}

// ---- shifted L1 ----
struct Taps {
    const int32_t* bx; const float* fx; const int32_t* by; const float* fy;
};

__device__ __forceinline__ float pix(const float* __restrict__ p, int H, int W, int y, int x, int clamp01) {
    if (y < 0 || y >= H || x < 0 || x >= W) return 0.f;
    const float v = p[(long long)y * W + x];
    return clamp01 ? clamp_unit(v) : v;
}

__device__ __forceinline__ float bilin(const float* __restrict__ p, int H, int W, int y0, float fy, int x0, float fx, int clamp01) {
    const float r0 = (1.f - fx) * pix(p, H, W, y0, x0, clamp01) + fx * pix(p, H, W, y0, x0 + 1, clamp01);
    const float r1 = (1.f - fx) * pix(p, H, W, y0 + 1, x0, clamp01) + fx * pix(p, H, W, y0 + 1, x0 + 1, clamp01);
    return (1.f - fy) * r0 + fy * r1;
}

__global__ __launch_bounds__(L_THREADS) void shift_l1_kernel(const float* __restrict__ x, int C, int H, int W, const float* __restrict__ mask, int nx, int ny,
                                                              Taps t, double* __restrict__ partial) {
    const int i = blockIdx.x, b = blockIdx.y;
    const long long plane = (long long)H * W;
    const float* img = x + (long long)b * C * plane;
    const int yp = t.by[i], ym = t.by[ny + i];
    const float fyp = t.fy[i], fym = t.fy[ny + i];
    double acc = 0.0;
    for (int j = threadIdx.x; j < nx; j += L_THREADS) {
        const int xp = t.bx[j], xm = t.bx[nx + j];
        const float fxp = t.fx[j], fxm = t.fx[nx + j];
        const float Mw = bilin(mask, H, W, yp, fyp, xp, fxp, 0) * bilin(mask, H, W, ym, fym, xm, fxm, 0);
        if (Mw == 0.f) continue;
        float s = 0.f;
        for (int c = 0; c < C; ++c) {
            const float* p = img + c * plane;
            s += fabsf(bilin(p, H, W, yp, fyp, xp, fxp, 1) - bilin(p, H, W, ym, fym, xm, fxm, 1));
        }
        acc += (double)(Mw * s);
    }
    __shared__ double red[1][L_THREADS];
    block_tree_sum(red, {acc});
    if (threadIdx.x == 0) partial[(long long)b * ny + i] = red[0][0];
}

// G[b][c][i][j] = g[b] M(i, j) sign(GS+ - GS-)   (torch's |.|' = 0 at 0)
__global__ __launch_bounds__(L_THREADS) void shift_l1_cot_kernel(const float* __restrict__ x, int C, int H, int W, const float* __restrict__ mask, int nx, int ny,
                                                                  Taps t, const float* __restrict__ g, float* __restrict__ G) {
    const int i = blockIdx.y, b = blockIdx.z;
    const int j = blockIdx.x * L_THREADS + threadIdx.x;
    if (j >= nx) return;
    const long long plane = (long long)H * W;
    const float* img = x + (long long)b * C * plane;
    const int yp = t.by[i], ym = t.by[ny + i], xp = t.bx[j], xm = t.bx[nx + j];
    const float fyp = t.fy[i], fym = t.fy[ny + i], fxp = t.fx[j], fxm = t.fx[nx + j];
    const float Mw = bilin(mask, H, W, yp, fyp, xp, fxp, 0) * bilin(mask, H, W, ym, fym, xm, fxm, 0) * g[b];
    for (int c = 0; c < C; ++c) {
        float r = 0.f;
        if (Mw != 0.f) {
            const float* p = img + c * plane;
            const float d = bilin(p, H, W, yp, fyp, xp, fxp, 1) - bilin(p, H, W, ym, fym, xm, fxm, 1);
            r = d > 0.f ? Mw : (d < 0.f ? -Mw : 0.f);
        }
        G[(((long long)b * C + c) * ny + i) * nx + j] = r;
    }
}

__device__ __forceinline__ float tap_w(int base, float frac, int s) { return base == s ? 1.f - frac : (base + 1 == s ? frac : 0.f); }

// dx[b][c][y][x] (+)= [0 <= x <= 1] sum_s sgn_s sum_{i in ry[s][y]} wy_s(i, y) sum_{j in rx[s][x]} wx_s(j, x) G[b][c][i][j]
__global__ __launch_bounds__(L_THREADS) void shift_l1_adj_kernel(const float* __restrict__ x, int C, int H, int W, int nx, int ny, Taps t,
                                                                  const int32_t* __restrict__ rx, const int32_t* __restrict__ ry, const float* __restrict__ G,
                                                                  float* __restrict__ dx, int accumulate) {
    const int y = blockIdx.y, b = blockIdx.z;
    const int xx = blockIdx.x * L_THREADS + threadIdx.x;
    if (xx >= W) return;
    const long long plane = (long long)H * W;
    int ilo[2], ihi[2], jlo[2], jhi[2];
    for (int s = 0; s < 2; ++s) {
        ilo[s] = max(ry[((long long)s * H + y) * 2], 0);
        ihi[s] = min(ry[((long long)s * H + y) * 2 + 1], ny);
        jlo[s] = max(rx[((long long)s * W + xx) * 2], 0);
        jhi[s] = min(rx[((long long)s * W + xx) * 2 + 1], nx);
    }
    for (int c = 0; c < C; ++c) {
        const float* Gc = G + ((long long)b * C + c) * ny * nx;
        float acc = 0.f;
        for (int s = 0; s < 2; ++s) {
            float as = 0.f;
            for (int i = ilo[s]; i < ihi[s]; ++i) {
                const float wy = tap_w(t.by[s * ny + i], t.fy[s * ny + i], y);
                if (wy == 0.f) continue;
                float r = 0.f;
                for (int j = jlo[s]; j < jhi[s]; ++j) {
                    const float wx = tap_w(t.bx[s * nx + j], t.fx[s * nx + j], xx);
                    r += wx * Gc[(long long)i * nx + j];
                }
                as += wy * r;
            }
            acc += s == 0 ? as : -as;
        }
        const long long off = ((long long)b * C + c) * plane + (long long)y * W + xx;
        gated_store(dx + off, x[off], acc, accumulate);
    }
}

}  // namespace

extern "C" int esr_patch_std(const float* x, int B, int C, int H, int W, const uint8_t* corners, float* S, float* mean, esr_stream_t stream) {
    if (!x || !corners || !S || !mean || B <= 0 || C <= 0 || H < LP || W < LP) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(patch_std_kernel, PT::corner_grid(B, H, W), dim3(L_THREADS), 0, (hipStream_t)stream, x, C, H, W, corners, S, mean);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_patch_std_grad(const float* x, int B, int C, int H, int W, const uint8_t* corners, const float* S, const float* mean, const float* dS,
                                  float* dx, int accumulate, esr_stream_t stream) {
    if (!x || !corners || !S || !mean || !dS || !dx || B <= 0 || C <= 0 || H < LP || W < LP) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(patch_std_grad_kernel, PT::pixel_grid(B, H, W), dim3(L_THREADS), 0, (hipStream_t)stream, x, C, H, W, corners, S, mean, dS, dx, accumulate);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_shift_l1(const float* x, int B, int C, int H, int W, const float* mask, int nx, int ny, const int32_t* base_x, const float* frac_x,
                            const int32_t* base_y, const float* frac_y, double* partial, esr_stream_t stream) {
    if (!x || !mask || !base_x || !frac_x || !base_y || !frac_y || !partial || B <= 0 || C <= 0 || H <= 0 || W <= 0 || nx <= 0 || ny <= 0) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    const Taps t{base_x, frac_x, base_y, frac_y};
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(shift_l1_kernel, dim3((unsigned)ny, (unsigned)B), dim3(L_THREADS), 0, (hipStream_t)stream, x, C, H, W, mask, nx, ny, t, partial);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_shift_l1_grad(const float* x, int B, int C, int H, int W, const float* mask, int nx, int ny, const int32_t* base_x, const float* frac_x,
                                 const int32_t* base_y, const float* frac_y, const int32_t* ranges_x, const int32_t* ranges_y, const float* g, float* work,
                                 float* dx, int accumulate, esr_stream_t stream) {
    if (!x || !mask || !base_x || !frac_x || !base_y || !frac_y || !ranges_x || !ranges_y || !g || !work || !dx || B <= 0 || C <= 0 || H <= 0 || W <= 0 ||
        nx <= 0 || ny <= 0)
        return ESR_E_ARG;
    if (!grid_ok(B, H, W) || ny > 65535) return ESR_E_UNSUPPORTED;
    const Taps t{base_x, frac_x, base_y, frac_y};
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(shift_l1_cot_kernel, dim3((unsigned)((nx + L_THREADS - 1) / L_THREADS), (unsigned)ny, (unsigned)B), dim3(L_THREADS), 0,
                       (hipStream_t)stream, x, C, H, W, mask, nx, ny, t, g, work);
    ESR_CHECK_LAUNCH();
    hipLaunchKernelGGL(shift_l1_adj_kernel, dim3((unsigned)((W + L_THREADS - 1) / L_THREADS), (unsigned)H, (unsigned)B), dim3(L_THREADS), 0,
                       (hipStream_t)stream, x, C, H, W, nx, ny, t, ranges_x, ranges_y, work, dx, accumulate);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
