// Patch-magnitude Z objective (reference codes/Z_optimization.py:391-394, 450-455, 717-722): the kernels behind the GUI's "increase / decrease
// variance" tool with its special-behaviour button checked ('local_Mag_increase' / 'local_Mag_decrease').
//
// For the P selected 7 x 7 windows of the gray image v_b = mean_c clamp(x_b, 0, 1) — the half-overlap patch set of
// ReturnPatchExtractionMat(image_mask, 7, patches_overlap=0.5), one corner in 16 to 27; esr_hip/patchmag.py builds it — and one desired
// patch per window (the initial output's patch with its STD moved by the increment), per image
//     sum_p sum_{k < 49} (v(window p, k) - desired[p][k])^2 ;
// the caller divides by 49 P.  The selection is an int32 map [H-6][W-6] of patch ordinals, -1 at unselected corners: with the map both
// directions run on the 22 x 70 patch-tile frame that csrc/esr_local.hip uses (Patch7 of csrc/esr_image.h: the tile load, the corner and pixel
// walks, the staging of the covering corners and the launch grids are that header's, not a copy), and a pixel finds the windows covering it
// without a cover list.
// The reference gathers the 49 x P values with torch.sparse.mm against a (49 P) x (H W) matrix per image.
// Forward: a workgroup reads a 22 x 70 tile of v into LDS (clamp and channel mean fused into the read) and every thread evaluates the
// selected corners among its four; float per window, double across windows, a fixed-order LDS reduction to partial[b][tile].  No atomics.
// Backward, gather form: with a_b = 2 g[b] / (49 P),
//     dv(y, x) = a_b sum over the selected corners (cy, cx) whose window covers (y, x) of (v(y, x) - desired[p][(y - cy) 7 + (x - cx)])
//     dx_c = dv / C [0 <= x_c <= 1]
// A workgroup owns a 16 x 64 pixel tile and stages the ordinals of the 22 x 70 corners covering it in LDS: no atomics, bit-reproducible.
// An ordinal outside [0, P) counts as unselected in both kernels (nothing is read through it).
#include "esr_image.h"

namespace {

using PT = Patch7;
constexpr int MP = PT::SIDE, MD = PT::AREA;  // patch side (the reference's PATCH_SIZE_4_STD) and entries per patch
constexpr int M_THREADS = PT::NT;

__global__ __launch_bounds__(M_THREADS) void patch_mag_kernel(const float* __restrict__ x, int C, int H, int W, const int32_t* __restrict__ index,
                                                                const float* __restrict__ desired, int P, double* __restrict__ partial) {
    __shared__ float v[PT::SY][PT::SX];
    __shared__ double red[1][M_THREADS];
    PT::load_gray(v, x, C, H, W);
    const int Wc = W - MP + 1;
    double acc = 0.0;
    PT::for_corners(H, W, [&](int cy, int cx, int ty, int tx) {
        const int p = index[(long long)cy * Wc + cx];
        if (p < 0 || p >= P) return;
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
    });
    block_tree_sum(red, {acc});
    if (threadIdx.x == 0) partial[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0][0];
}

__global__ __launch_bounds__(M_THREADS) void patch_mag_grad_kernel(const float* __restrict__ x, int C, int H, int W, const int32_t* __restrict__ index,
                                                                     const float* __restrict__ desired, int P, const float* __restrict__ g,
                                                                     float* __restrict__ dx, int accumulate) {
    __shared__ int32_t ord[PT::SY][PT::SX];
    const int b = blockIdx.z, Wc = W - MP + 1;
    const long long plane = (long long)H * W;
    PT::stage_corners(H, W, [&](int ty, int tx, int cy, int cx, bool inside) {
        int32_t p = -1;
        if (inside) {
            p = index[(long long)cy * Wc + cx];
            if (p >= P) p = -1;
        }
        ord[ty][tx] = p;
    });
    const float* img = x + (long long)b * C * plane;
    float* out = dx + (long long)b * C * plane;
    PT::for_pixels(H, W, [&](int y, int xx, int ty, int tx) {
        const float a = 2.f * g[b] / ((float)MD * (float)P);
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
        gated_store_pixel(out, img, C, plane, off, a * acc / (float)C, accumulate);
    });
}

}  // namespace

extern "C" int64_t esr_patch_mag_blocks(int H, int W) {
    if (H < MP || W < MP) return 0;
    const dim3 grid = PT::corner_grid(1, H, W);
    return (int64_t)grid.y * grid.x;
}

extern "C" int esr_patch_mag(const float* x, int B, int C, int H, int W, const int32_t* corner_index, const float* desired, int P, double* partial,
                             esr_stream_t stream) {
    if (!x || !corner_index || !desired || !partial || B <= 0 || C <= 0 || H < MP || W < MP || P <= 0) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(patch_mag_kernel, PT::corner_grid(B, H, W), dim3(M_THREADS), 0, (hipStream_t)stream, x, C, H, W, corner_index, desired, P, partial);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

extern "C" int esr_patch_mag_grad(const float* x, int B, int C, int H, int W, const int32_t* corner_index, const float* desired, int P, const float* g,
                                  float* dx, int accumulate, esr_stream_t stream) {
    if (!x || !corner_index || !desired || !g || !dx || B <= 0 || C <= 0 || H < MP || W < MP || P <= 0) return ESR_E_ARG;
    if (!grid_ok(B, H, W)) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    hipLaunchKernelGGL(patch_mag_grad_kernel, PT::pixel_grid(B, H, W), dim3(M_THREADS), 0, (hipStream_t)stream, x, C, H, W, corner_index, desired, P, g, dx, accumulate);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
