// Scribble Z objective with its region constraint (reference codes/Z_optimization.py:344-364, 385-390, 401-448, 743-746): the kernels behind
// the GUI's Draw, brightness +/- brush, local-TV brush and imprint tools, all of which send 'scribble' with non_local_Z_optimization on.
//
// Per image b of v = clamp(x_b, 0, 1), with one label byte per pixel (esr_hip/scribble.py builds it: bit 7 the L1 set, bit 6 the constraint
// set 1 - (image_mask > 0), bits 0-5 a TV region id T, 0 = none):
//     l1     = sum_{c,p in L1} |v(c,p) - D(c,p)|
//     tv_d   = sum_{c,p} [T(p) = T(p + d) > 0] |v(c,p) - v(c,p + d)|   for d = (1,1) and (-1,1)    (diagonal pairs, one sum)
//     tv_v   = the same for d = (1,0),   tv_h = the same for d = (0,1)                            (d = (dy, dx), p + d inside the image)
//     con    = sum_{c,p in constraint} |v(c,p) - I0(c,p)|                                           (I0: the initial output, batch 1 or B)
// One label map serves any number of TV regions: they are disjoint, so sum_k R_k(p) R_k(p + d) = [T(p) = T(p + d) > 0].  The reference's
// per-region, per-offset torch passes (4 k + 3 full-size passes for k regions) become one read of x.
// Forward: a workgroup per (row, image) writes partial[b][y][5] = (l1, tv_d, tv_v, tv_h, con) as doubles (per-thread double sums, a fixed-order
// LDS reduction; the caller sums the rows).  No atomics, bit-reproducible.
// Backward, gather form: pixel q collects its own L1 and constraint terms and the 8 pair terms in which it is the first or the second element;
// both give + w sign(v(q) - v(n)) for the neighbour n, w the offset class's weight.  No atomics.
#include "esr_image.h"

namespace {

constexpr int S_THREADS = 256;
constexpr uint8_t LAB_L1 = 0x80, LAB_CON = 0x40, LAB_TV = 0x3f;

__global__ __launch_bounds__(S_THREADS) void scribble_kernel(const float* __restrict__ x, int C, int H, int W, const float* __restrict__ D,
                                                              const uint8_t* __restrict__ lab, const float* __restrict__ i0, int i0_batch,
                                                              double* __restrict__ partial) {
    const int y = blockIdx.x, b = blockIdx.y;
    const long long plane = (long long)H * W;
    const float* img = x + (long long)b * C * plane;
    const float* ref = i0 ? i0 + (i0_batch == 1 ? 0 : (long long)b * C * plane) : nullptr;
    const uint8_t* row = lab + (long long)y * W;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int xx = threadIdx.x; xx < W; xx += S_THREADS) {
        const uint8_t l = row[xx];
        if (!l) continue;
        const int t = l & LAB_TV;
        const bool con = (l & LAB_CON) && ref;
        // the neighbours that pair with this pixel as the first element (same region id)
        const bool r = xx + 1 < W, up = y > 0, dn = y + 1 < H;
        const bool m_dr = t && dn && r && (row[W + xx + 1] & LAB_TV) == t;     // d = (1, 1)
        const bool m_ur = t && up && r && (row[xx + 1 - W] & LAB_TV) == t;     // d = (-1, 1)
        const bool m_d = t && dn && (row[W + xx] & LAB_TV) == t;               // d = (1, 0)
        const bool m_r = t && r && (row[xx + 1] & LAB_TV) == t;                // d = (0, 1)
        const long long o = (long long)y * W + xx;
        float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            const float* p = img + c * plane + o;
            const float v = clamp_unit(*p);
            if (l & LAB_L1) a[0] += fabsf(v - D[c * plane + o]);
            if (m_dr) a[1] += fabsf(v - clamp_unit(p[W + 1]));
            if (m_ur) a[1] += fabsf(v - clamp_unit(p[1 - W]));
            if (m_d) a[2] += fabsf(v - clamp_unit(p[W]));
            if (m_r) a[3] += fabsf(v - clamp_unit(p[1]));
            if (con) a[4] += fabsf(v - ref[c * plane + o]);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += (double)a[k];
    }
    __shared__ double red[5][S_THREADS];
    block_tree_sum(red, s);
    if (threadIdx.x < 5) partial[((long long)b * H + y) * 5 + threadIdx.x] = red[threadIdx.x][0];
}

// dx[b][c][y][x] (+)= [0 <= x <= 1] ( g[b] (w_l1 [L1] sign(v - D) + sum_{n in N8, T(n) = T(q) > 0} w_n sign(v - v_n)) + g_con [con] sign(v - I0) )
__global__ __launch_bounds__(S_THREADS) void scribble_grad_kernel(const float* __restrict__ x, int C, int H, int W, const float* __restrict__ D,
                                                                   const uint8_t* __restrict__ lab, const float* __restrict__ i0, int i0_batch,
                                                                   const float* __restrict__ g, float g_con, float* __restrict__ dx, int accumulate) {
    const int y = blockIdx.y, b = blockIdx.z;
    const int xx = blockIdx.x * S_THREADS + threadIdx.x;
    if (xx >= W) return;
    const long long plane = (long long)H * W;
    const long long o = (long long)y * W + xx;
    const float* img = x + (long long)b * C * plane;
    float* out = dx + (long long)b * C * plane;
    const float* ref = i0 ? i0 + (i0_batch == 1 ? 0 : (long long)b * C * plane) : nullptr;
    const uint8_t l = lab[o];
    const int t = l & LAB_TV;
    const bool con = (l & LAB_CON) && ref;
    // the term weights of L_b = l1 / (C H W) + tv_d / (C (H-1)(W-1)) + tv_v / (C (H-1) W) + tv_h / (C H (W-1)), times g[b]
    const float gb = g[b];
    const float w_l1 = gb / ((float)C * H * W);
    const float w_d = H > 1 && W > 1 ? gb / ((float)C * (H - 1) * (W - 1)) : 0.f;
    const float w_v = H > 1 ? gb / ((float)C * (H - 1) * W) : 0.f;
    const float w_h = W > 1 ? gb / ((float)C * H * (W - 1)) : 0.f;
    // neighbour n = q + (dy, dx) with the same region id: bit k of `nb`, k counting the 8 offsets row-major (the centre skipped)
    unsigned nb = 0;
    if (t) {
        int k = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dxx = -1; dxx <= 1; ++dxx) {
                if (dy == 0 && dxx == 0) continue;
                const int ny = y + dy, nx = xx + dxx;
                if (ny >= 0 && ny < H && nx >= 0 && nx < W && (lab[(long long)ny * W + nx] & LAB_TV) == t) nb |= 1u << k;
                ++k;
            }
    }
    for (int c = 0; c < C; ++c) {
        const float* p = img + c * plane + o;
        const float raw = *p;
        const float v = clamp_unit(raw);
        float acc = 0.f;
        if (l & LAB_L1) acc += w_l1 * sgn(v - D[c * plane + o]);
        if (nb) {
            int k = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dxx = -1; dxx <= 1; ++dxx) {
                    if (dy == 0 && dxx == 0) continue;
                    if (nb >> k & 1u) acc += (dy == 0 ? w_h : (dxx == 0 ? w_v : w_d)) * sgn(v - clamp_unit(p[dy * W + dxx]));
                    ++k;
                }
        }
        if (con) acc += g_con * sgn(v - ref[c * plane + o]);
        gated_store(out + c * plane + o, raw, acc, accumulate);
    }
}

}  // namespace

extern "C" int esr_scribble(const float* x, int B, int C, int H, int W, const float* desired, const uint8_t* labels, const float* i0, int i0_batch,
                            double* partial, esr_stream_t stream) {
    if (!x || !desired || !labels || !partial || B <= 0 || C <= 0 || H <= 0 || W <= 0) return ESR_E_ARG;
    if (i0 && i0_batch != 1 && i0_batch != B) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(scribble_kernel, dim3((unsigned)H, (unsigned)B), dim3(S_THREADS), 0, (hipStream_t)stream, x, C, H, W, desired, labels, i0,
                       i0_batch, partial);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_scribble_grad(const float* x, int B, int C, int H, int W, const float* desired, const uint8_t* labels, const float* i0, int i0_batch,
                                 const float* g, float g_con, float* dx, int accumulate, esr_stream_t stream) {
    if (!x || !desired || !labels || !g || !dx || B <= 0 || C <= 0 || H <= 0 || W <= 0) return ESR_E_ARG;
    if (i0 && i0_batch != 1 && i0_batch != B) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(scribble_grad_kernel, dim3((unsigned)((W + S_THREADS - 1) / S_THREADS), (unsigned)H, (unsigned)B), dim3(S_THREADS), 0,
                       (hipStream_t)stream, x, C, H, W, desired, labels, i0, i0_batch, g, g_con, dx, accumulate);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
