// Patch-magnitude Z objective (reference codes/Z_optimization.py:391-394, 450-455, 717-722): the kernels behind the GUI's "increase / decrease
// variance" tool with its special-behaviour button checked ('local_Mag_increase' / 'local_Mag_decrease').
//
// For the P selected 7 x 7 windows of the gray image v_b = mean_c clamp(x_b, 0, 1) — the half-overlap patch set of
// ReturnPatchExtractionMat(image_mask, 7, patches_overlap=0.5), one corner in 16 to 27; esr_hip/patchmag.py builds it — and one desired
// patch per window (the initial output's patch with its STD moved by the increment), per image
//     sum_p sum_{k < 49} (v(window p, k) - desired[p][k])^2 ;
// the caller divides by 49 P.  The selection is an int32 map [H-6][W-6] of patch ordinals, -1 at unselected corners: the map keeps the
// 22 x 70 LDS tiling of csrc/esr_local.hip unchanged in both directions, and a pixel finds the windows covering it without a cover list.
// The reference gathers the 49 x P values with torch.sparse.mm against a (49 P) x (H W) matrix per image.
// Forward: a workgroup reads a 22 x 70 tile of v into LDS (clamp and channel mean fused into the read) and every thread evaluates the
// selected corners among its four; float per window, double across windows, a fixed-order LDS reduction to partial[b][tile].  No atomics.
// Backward, gather form: with a_b = 2 g[b] / (49 P),
//     dv(y, x) = a_b sum over the selected corners (cy, cx) whose window covers (y, x) of (v(y, x) - desired[p][(y - cy) 7 + (x - cx)])
//     dx_c = dv / C [0 <= x_c <= 1]
// A workgroup owns a 16 x 64 pixel tile and stages the ordinals of the 22 x 70 corners covering it in LDS: no atomics, bit-reproducible.
// An ordinal outside [0, P) counts as unselected in both kernels (nothing is read through it).
#include "esr_common.h"

namespace {

constexpr int MP = 7;                        // patch side (the reference's PATCH_SIZE_4_STD)
constexpr int MD = MP * MP;
constexpr int MT_X = 64, MT_Y = 16;          // corner / pixel tile per workgroup
constexpr int MS_X = MT_X + MP - 1, MS_Y = MT_Y + MP - 1;
constexpr int M_THREADS = 256;

__global__ __launch_bounds__(M_THREADS) void patch_mag_kernel(const float* __restrict__ x, int C, int H, int W, const int32_t* __restrict__ index,
                                                                const float* __restrict__ desired, int P, double* __restrict__ partial) {
    __shared__ float v[MS_Y][MS_X];
    __shared__ double red[M_THREADS];
    const int b = blockIdx.z, cy0 = blockIdx.y * MT_Y, cx0 = blockIdx.x * MT_X;
    const int Hc = H - MP + 1, Wc = W - MP + 1;
    const long long plane = (long long)H * W;
    const float* img = x + (long long)b * C * plane;
    for (int t = threadIdx.x; t < MS_Y * MS_X; t += M_THREADS) {
        const int ty = t / MS_X, tx = t % MS_X, y = cy0 + ty, xx = cx0 + tx;
        v[ty][tx] = (y < H && xx < W) ? gray(img, C, plane, (long long)y * W + xx) : 0.f;
    }
    __syncthreads();
    const int tx = threadIdx.x % MT_X;
    const int cx = cx0 + tx;
    double acc = 0.0;
    if (cx < Wc) {
        for (int ty = threadIdx.x / MT_X; ty < MT_Y; ty += M_THREADS / MT_X) {
            const int cy = cy0 + ty;
            if (cy >= Hc) break;
            const int p = index[(long long)cy * Wc + cx];
            if (p < 0 || p >= P) continue;
            const float* d = desired + (long long)p * MD;
            float s = 0.f;
#pragma unroll
            for (int dy = 0; dy < MP; ++dy)
#pragma unroll
                for (int dx = 0; dx < MP; ++dx) {
                    const float e = v[ty + dy][tx + dx] - d[dy * MP + dx];
                    s += e * e;
                }
            acc += (double)s;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = M_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(M_THREADS) void patch_mag_grad_kernel(const float* __restrict__ x, int C, int H, int W, const int32_t* __restrict__ index,
                                                                     const float* __restrict__ desired, int P, const float* __restrict__ g,
                                                                     float* __restrict__ dx, int accumulate) {
    __shared__ int32_t ord[MS_Y][MS_X];
    const int b = blockIdx.z, y0 = blockIdx.y * MT_Y, x0 = blockIdx.x * MT_X;
    const int Hc = H - MP + 1, Wc = W - MP + 1;
    const long long plane = (long long)H * W;
    for (int t = threadIdx.x; t < MS_Y * MS_X; t += M_THREADS) {
        const int ty = t / MS_X, tx = t % MS_X, cy = y0 - (MP - 1) + ty, cx = x0 - (MP - 1) + tx;
        int32_t p = -1;
        if (cy >= 0 && cx >= 0 && cy < Hc && cx < Wc) {
            p = index[(long long)cy * Wc + cx];
            if (p >= P) p = -1;
        }
        ord[ty][tx] = p;
    }
    __syncthreads();
    const int tx = threadIdx.x % MT_X;
    const int xx = x0 + tx;
    if (xx >= W) return;
    const float* img = x + (long long)b * C * plane;
    float* out = dx + (long long)b * C * plane;
    const float a = 2.f * g[b] / ((float)MD * (float)P);
    for (int ty = threadIdx.x / MT_X; ty < MT_Y; ty += M_THREADS / MT_X) {
        const int y = y0 + ty;
        if (y >= H) break;
        const long long off = (long long)y * W + xx;
        const float v = gray(img, C, plane, off);
        float acc = 0.f;
        // the corner at tile offset (ty + j, tx + i) is (y - 6 + j, x - 6 + i): this pixel is its window's entry (6 - j, 6 - i)
#pragma unroll
        for (int j = 0; j < MP; ++j)
#pragma unroll
            for (int i = 0; i < MP; ++i) {
                const int32_t p = ord[ty + j][tx + i];
                if (p >= 0) acc += v - desired[(long long)p * MD + (MP - 1 - j) * MP + (MP - 1 - i)];
            }
        const float gv = a * acc / (float)C;
        for (int c = 0; c < C; ++c) {
            const float raw = img[c * plane + off];
            const float gc = (raw >= 0.f && raw <= 1.f) ? gv : 0.f;      // torch.clamp's gradient: 1 inside and at the bounds
            float* o = out + c * plane + off;
            *o = accumulate ? *o + gc : gc;
        }
    }
}

bool grid_ok(int B, int H, int W) { return B <= 65535 && H <= 65535 && W <= 65535; }

}  // namespace

extern "C" int64_t esr_patch_mag_blocks(int H, int W) {
    if (H < MP || W < MP) return 0;
    return (int64_t)((H - MP + 1 + MT_Y - 1) / MT_Y) * ((W - MP + 1 + MT_X - 1) / MT_X);
}

extern "C" int esr_patch_mag(const float* x, int B, int C, int H, int W, const int32_t* corner_index, const float* desired, int P, double* partial,
                             esr_stream_t stream) {
    if (!x || !corner_index || !desired || !partial || B <= 0 || C <= 0 || H < MP || W < MP || P <= 0) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    const int Hc = H - MP + 1, Wc = W - MP + 1;
    const dim3 grid((unsigned)((Wc + MT_X - 1) / MT_X), (unsigned)((Hc + MT_Y - 1) / MT_Y), (unsigned)B);
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(patch_mag_kernel, grid, dim3(M_THREADS), 0, (hipStream_t)stream, x, C, H, W, corner_index, desired, P, partial);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_patch_mag_grad(const float* x, int B, int C, int H, int W, const int32_t* corner_index, const float* desired, int P, const float* g,
                                  float* dx, int accumulate, esr_stream_t stream) {
    if (!x || !corner_index || !desired || !g || !dx || B <= 0 || C <= 0 || H < MP || W < MP || P <= 0) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    const dim3 grid((unsigned)((W + MT_X - 1) / MT_X), (unsigned)((H + MT_Y - 1) / MT_Y), (unsigned)B);
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(patch_mag_grad_kernel, grid, dim3(M_THREADS), 0, (hipStream_t)stream, x, C, H, W, corner_index, desired, P, g, dx, accumulate);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
