// Shared device helpers of the image-space Z-objective kernels (esr_local, esr_patchmag, esr_scribble, esr_zobj, esr_pairmin): the clamp gate
// of their backward passes, the fixed-order block reduction of their forward passes, and the 7 x 7 patch-tile frame of the patch objectives.
// The scalar helpers they build on (clamp_unit, sgn, gray, clampi) are esr_common.h's.
#pragma once
#include "esr_common.h"

// ---- the clamp gate: d clamp(x, 0, 1) / dx
// torch.clamp's gradient: 1 inside and AT the bounds ((x >= min) & (x <= max)), 0 outside (NaN: 0)
__device__ __forceinline__ bool clamp_gate(float raw) { return raw >= 0.f && raw <= 1.f; }
// *o (+)= [0 <= raw <= 1] g
__device__ __forceinline__ void gated_store(float* o, float raw, float g, int accumulate) {
    const float gc = clamp_gate(raw) ? g : 0.f;
    *o = accumulate ? *o + gc : gc;
}
// the same for the C channels of one pixel (planes `plane` apart) that share the gradient g of their gray value
__device__ __forceinline__ void gated_store_pixel(float* out, const float* __restrict__ img, int C, long long plane, long long off, float g, int accumulate) {
    for (int c = 0; c < C; ++c) gated_store(out + c * plane + off, img[c * plane + off], g, accumulate);
}

// ---- fixed-order LDS tree reduction of K doubles per thread over the N threads of a workgroup (halving stride, thread t adds t + w): the
// sums are left in red[k][0], visible to every thread on return.  No atomics, so two runs are bit-identical.
template <int N, int K>
__device__ __forceinline__ void block_tree_sum(double (&red)[K][N], const double (&s)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int w = N / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        __syncthreads();
    }
}

// launch grids index images and image rows with blockIdx.y / .z
static inline bool grid_ok(int B, int H, int W) { return B <= 65535 && H <= 65535 && W <= 65535; }

// ---- the patch-tile frame: P x P windows named by their top-left corner, Hc x Wc = (H - P + 1) x (W - P + 1) corners per image.
// A workgroup of THREADS (a multiple of TX) owns a TY x TX tile of corners (forward) or of pixels (backward), blockIdx = (tile x, tile y, image).
// Forward: the (TY + P - 1) x (TX + P - 1) pixels under the tile's windows go to LDS once (load_gray), then every thread visits its corners
// (for_corners).  Backward, gather form: the (TY + P - 1) x (TX + P - 1) corners whose windows cover the pixel tile are staged in LDS
// (stage_corners: tile entry (ty, tx) is corner (y0 - (P - 1) + ty, x0 - (P - 1) + tx)), then every thread visits its pixels (for_pixels): pixel
// tile offset (ty, tx) is entry (P - 1 - j, P - 1 - i) of the window at tile entry (ty + j, tx + i).  A kernel supplies its arithmetic as functors.
template <int P, int TX, int TY, int THREADS>
struct PatchTile {
    static constexpr int SIDE = P, AREA = P * P, SX = TX + P - 1, SY = TY + P - 1, NT = THREADS;

    static dim3 grid(int B, int rows, int cols) { return dim3((unsigned)((cols + TX - 1) / TX), (unsigned)((rows + TY - 1) / TY), (unsigned)B); }
    static dim3 corner_grid(int B, int H, int W) { return grid(B, H - P + 1, W - P + 1); }
    static dim3 pixel_grid(int B, int H, int W) { return grid(B, H, W); }

    // v = the gray image of this block's image under its corner tile, 0 beyond the image; ends with a barrier
    __device__ static __forceinline__ void load_gray(float (&v)[SY][SX], const float* __restrict__ x, int C, int H, int W) {
        const int cy0 = blockIdx.y * TY, cx0 = blockIdx.x * TX;
        const long long plane = (long long)H * W;
        const float* img = x + (long long)blockIdx.z * C * plane;
        for (int t = threadIdx.x; t < SY * SX; t += THREADS) {
            const int ty = t / SX, tx = t % SX, y = cy0 + ty, xx = cx0 + tx;
            v[ty][tx] = (y < H && xx < W) ? gray(img, C, plane, (long long)y * W + xx) : 0.f;
        }
        __syncthreads();
    }

    // f(cy, cx, ty, tx) for this thread's corners inside Hc x Wc: the window of corner (cy, cx) is v[ty .. ty + P - 1][tx .. tx + P - 1]
    template <typename F>
    __device__ static __forceinline__ void for_corners(int H, int W, F f) {
        const int Hc = H - P + 1, Wc = W - P + 1;
        const int tx = threadIdx.x % TX, cx = blockIdx.x * TX + tx;
        if (cx >= Wc) return;
        for (int ty = threadIdx.x / TX; ty < TY; ty += THREADS / TX) {
            const int cy = blockIdx.y * TY + ty;
            if (cy >= Hc) break;
            f(cy, cx, ty, tx);
        }
    }

    // f(ty, tx, cy, cx, inside) for the SY x SX corners covering this block's pixel tile, `inside`: the corner exists; f stores what the
    // kernel keeps per corner at [ty][tx] of its LDS arrays.  Ends with a barrier.
    template <typename F>
    __device__ static __forceinline__ void stage_corners(int H, int W, F f) {
        const int Hc = H - P + 1, Wc = W - P + 1;
        const int y0 = blockIdx.y * TY, x0 = blockIdx.x * TX;
        for (int t = threadIdx.x; t < SY * SX; t += THREADS) {
            const int ty = t / SX, tx = t % SX, cy = y0 - (P - 1) + ty, cx = x0 - (P - 1) + tx;
            f(ty, tx, cy, cx, cy >= 0 && cx >= 0 && cy < Hc && cx < Wc);
        }
        __syncthreads();
    }

    // f(y, xx, ty, tx) for this thread's pixels inside H x W
    template <typename F>
    __device__ static __forceinline__ void for_pixels(int H, int W, F f) {
        const int tx = threadIdx.x % TX, xx = blockIdx.x * TX + tx;
        if (xx >= W) return;
        for (int ty = threadIdx.x / TX; ty < TY; ty += THREADS / TX) {
            const int y = blockIdx.y * TY + ty;
            if (y >= H) break;
            f(y, xx, ty, tx);
        }
    }
};

// the 7 x 7 patches of the local-STD and patch-magnitude objectives (the reference's PATCH_SIZE_4_STD): 22 x 70 LDS tiles, 256 threads
using Patch7 = PatchTile<7, 64, 16, 256>;
