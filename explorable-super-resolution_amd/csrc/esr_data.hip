// LR/HR training batches synthesised on the device from resident uint8 images — what the reference's LRHRDataset.__getitem__ does per item on the
// host (codes/data/LRHR_dataset.py:48-131: read_img's /255, channel_convert, CEM imresize of the WHOLE image, the random crop, util.augment, BGR->RGB,
// HWC->CHW) and its DataLoader then collates and copies.  One launch makes hr[B][Co][ph][pw] and lr[B][Co][ph/sf][pw/sf].
//
// A workgroup owns a T x T tile of LR crop pixels of one item, i.e. a (T sf)^2 tile of its HR crop.  It stages the source window both need —
// `lo` pixels above/left of the HR tile, `win` a side (data_plan) — once in LDS, every coordinate clamped to the item's LOGICAL image (replicate
// padding of the whole image, never of the crop): as bytes, one plane per channel, for the "BGR->RGB, /255" map; as converted fp32 for the 3->1
// mix, which is applied per source pixel before filtering, as the reference converts img_HR before imresize.  From the window it writes
//   * the HR tile: byte / 255 as an IEEE fp32 division (bit-identical to u8.astype(float32) / 255.), or the mixed value;
//   * the LR tile: sum_{u,v} taps[u][v] window[pre + sf i + half - u][pre + sf j + half - v] in fp32, u outer, v inner.  On byte windows the sum
//     runs over the bytes and is divided by 255 once at the end;
// or, for an item that brings its own LR image, the plain crop of that image through the same channel map.  The augmentation (hflip, vflip,
// transpose, in util.augment's order) is a mapping of the OUTPUT index: threads enumerate the tile in output order, so that stores stay coalesced
// under a transpose and the strided side is the LDS read.  The source is read from HBM once per tile (halo re-reads hit L2); plain vector loads and
// stores only; the taps are read at wave-uniform addresses.
#include "esr_common.h"

namespace {

constexpr int DT_THREADS = 256;
constexpr int DT_LDS_BUDGET = 64 * 1024;         // per workgroup: at least two workgroups per CU (160 KiB), and no dynamic-LDS attribute to raise
constexpr int DT_MAX_TILE = 8;                   // small tiles: a batch of 32 crops is then ~1500 short workgroups, six or more resident per CU
constexpr int DT_STAGE = 4;                      // window pixels a thread loads before it stores the first

// ---- launch plan: decided from (sf, k, pre) alone
struct DataPlan {
    int tile;       // T: LR pixels a side per workgroup
    int lo;         // window rows / columns before the HR tile's first
    int win;        // window side, source pixels
};

static int data_window(int T, int sf, int k, int pre, int& lo) {
    const int half = k / 2;
    lo = half > pre ? half - pre : 0;
    const int hr_side = T * sf, lr_reach = (T - 1) * sf + pre + half + 1;
    return lo + (hr_side > lr_reach ? hr_side : lr_reach);
}

// the largest power-of-two tile up to 8 whose window fits the budget at 4 bytes per pixel (fp32 of the mix; three byte planes need less)
static bool data_plan(int sf, int k, int pre, DataPlan& p) {
    for (int T = DT_MAX_TILE; T >= 1; T >>= 1) {
        int lo;
        const long long win = data_window(T, sf, k, pre, lo);
        if (win * win * 4 <= DT_LDS_BUDGET) {
            p.tile = T;
            p.lo = lo;
            p.win = (int)win;
            return true;
        }
    }
    return false;
}

struct Mix { double w0, w1, w2, b, scale; };

// read_img's conversion: an IEEE division (u8.astype(float32) / 255.)
__device__ __forceinline__ float unit(uint8_t v) { return __fdiv_rn((float)v, 255.f); }

// ((dot(scale x, w)) / scale + b) / scale of a BGR pixel: the fp32 product scale x, then fp64, as util.bgr2ycbcr evaluates it on a float32 image
__device__ __forceinline__ float mix_pixel(const uint8_t* __restrict__ px, const Mix& m) {
    const float s = (float)m.scale;
    const double t0 = (double)(unit(px[0]) * s), t1 = (double)(unit(px[1]) * s), t2 = (double)(unit(px[2]) * s);
    const double acc = __dadd_rn(__dadd_rn(__dmul_rn(t0, m.w0), __dmul_rn(t1, m.w1)), __dmul_rn(t2, m.w2));      // left to right, no contraction
    return (float)((acc / m.scale + m.b) / m.scale);
}

// crop coordinate (cy, cx) -> output coordinate under util.augment's hflip, then vflip, then transpose (n0 x n1 crop; transposed crops are square)
__device__ __forceinline__ long long aug_offset(int cy, int cx, int n0, int n1, int flags) {
    const int fy = (flags & ESR_DATA_VFLIP) ? n0 - 1 - cy : cy;
    const int fx = (flags & ESR_DATA_HFLIP) ? n1 - 1 - cx : cx;
    return (flags & ESR_DATA_TRANSPOSE) ? (long long)fx * n1 + fy : (long long)fy * n1 + fx;
}

template <bool MIX>
__global__ __launch_bounds__(DT_THREADS) void lrhr_batch_kernel(const esr_data_item* __restrict__ items, DataPlan plan, int tiles_x, int sf, int k, int pre,
                                                                const float* __restrict__ taps, int ph, int pw, int Co, Mix mix,
                                                                float* __restrict__ hr, float* __restrict__ lr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* const winf = reinterpret_cast<float*>(smem);      // MIX: [win][win] converted values
    uint8_t* const winb = smem;                              // else: [Cs][win][win] bytes
    const int tid = threadIdx.x, b = blockIdx.y;
    const esr_data_item it = items[b];
    const int T = plan.tile, lo = plan.lo, Wn = plan.win, WW = Wn * Wn;
    const int ti = blockIdx.x / tiles_x, tj = blockIdx.x % tiles_x;
    const int lh = ph / sf, lw = pw / sf, half = k / 2;
    const int Cs = it.channels == 3 ? 3 : 1;
    const bool transpose = (it.flags & ESR_DATA_TRANSPOSE) != 0;

    // ---- stage the window: source rows r0 ... r0 + win - 1, clamped to the logical image
    const int r0 = it.y0 + ti * T * sf - lo, c0 = it.x0 + tj * T * sf - lo;
    // (DT_STAGE pixels per thread in flight: all their loads are issued before the first conversion or LDS store)
    for (int e0 = tid; e0 < WW; e0 += DT_THREADS * DT_STAGE) {
        uint8_t raw[DT_STAGE][3];
#pragma unroll
        for (int j = 0; j < DT_STAGE; ++j) {
            const int e = e0 + j * DT_THREADS;
            if (e >= WW) break;
            const int wr = e / Wn, wc = e - wr * Wn;
            const int sy = clampi(r0 + wr, 0, it.H - 1), sx = clampi(c0 + wc, 0, it.W - 1);
            const uint8_t* px = it.hr + ((long long)sy * it.stride + sx) * Cs;
            raw[j][0] = px[0];
            if (Cs == 3) {
                raw[j][1] = px[1];
                raw[j][2] = px[2];
            }
        }
#pragma unroll
        for (int j = 0; j < DT_STAGE; ++j) {
            const int e = e0 + j * DT_THREADS;
            if (e >= WW) break;
            if (MIX) {
                winf[e] = Cs == 3 ? mix_pixel(raw[j], mix) : unit(raw[j][0]);
            } else {
                for (int c = 0; c < Cs; ++c) winb[c * WW + e] = raw[j][c];
            }
        }
    }
    __syncthreads();

    // ---- the HR tile, enumerated in output order
    const int Ts = T * sf;
    for (int e = tid; e < Ts * Ts; e += DT_THREADS) {
        const int a = e / Ts, bb = e - a * Ts;
        const int ty = transpose ? bb : a, tx = transpose ? a : bb;
        const int cy = ti * Ts + ty, cx = tj * Ts + tx;
        if (cy >= ph || cx >= pw) continue;
        const int w = (lo + ty) * Wn + lo + tx;
        const long long o = aug_offset(cy, cx, ph, pw, it.flags);
        for (int c = 0; c < Co; ++c) {
            const float v = MIX ? winf[w] : unit(winb[(Cs == 3 ? 2 - c : 0) * WW + w]);          // BGR -> RGB
            hr[((long long)b * Co + c) * ph * pw + o] = v;
        }
    }

    // ---- the LR tile
    for (int e = tid; e < Co * T * T; e += DT_THREADS) {
        const int c = e / (T * T), r = e - c * T * T;
        const int a = r / T, bb = r - a * T;
        const int ty = transpose ? bb : a, tx = transpose ? a : bb;
        const int cy = ti * T + ty, cx = tj * T + tx;
        if (cy >= lh || cx >= lw) continue;
        const int cs = Cs == 3 ? 2 - c : 0;
        float v;
        if (it.lr) {                                          // a supplied LR image: its plain crop
            const int sy = clampi(it.y0 / sf + cy, 0, it.lr_H - 1), sx = clampi(it.x0 / sf + cx, 0, it.lr_W - 1);
            const uint8_t* px = it.lr + ((long long)sy * it.lr_stride + sx) * Cs;
            v = (MIX && Cs == 3) ? mix_pixel(px, mix) : unit(px[MIX ? 0 : cs]);
        } else {
            const int base = (pre + sf * ty + half + lo) * Wn + (pre + sf * tx + half + lo);
            float acc = 0.f;
            if (MIX) {
                for (int u = 0; u < k; ++u)
#pragma unroll 8
                    for (int x = 0; x < k; ++x) acc = fmaf(taps[u * k + x], winf[base - u * Wn - x], acc);
                v = acc;
            } else {
                const uint8_t* p = winb + cs * WW;
                for (int u = 0; u < k; ++u)
#pragma unroll 8
                    for (int x = 0; x < k; ++x) acc = fmaf(taps[u * k + x], (float)p[base - u * Wn - x], acc);
                v = __fdiv_rn(acc, 255.f);
            }
        }
        lr[((long long)b * Co + c) * lh * lw + aug_offset(cy, cx, lh, lw, it.flags)] = v;
    }
}

}  // namespace

extern "C" int esr_data_lrhr_plan(int sf, int k, int pre, int32_t* tile_lo_win) {
    if (sf < 1 || k < 1 || k > 63 || !(k & 1) || pre < 0 || pre >= sf || !tile_lo_win) return ESR_E_ARG;
    DataPlan p;
    if (!data_plan(sf, k, pre, p)) return ESR_E_UNSUPPORTED;
    tile_lo_win[0] = p.tile;
    tile_lo_win[1] = p.lo;
    tile_lo_win[2] = p.win;
    return ESR_OK;
}

extern "C" int esr_data_lrhr_batch(const esr_data_item* items, const esr_data_item* items_dev, int B, int sf, const float* taps, int k, int pre, int ph,
                                   int pw, const esr_data_channel_map* map, float* hr, float* lr, esr_stream_t stream) {
    if (!items || !items_dev || !map || !hr || !lr || B < 1 || sf < 1 || ph < 1 || pw < 1) return ESR_E_ARG;
    if (ph % sf || pw % sf || k < 1 || k > 63 || !(k & 1) || pre < 0 || pre >= sf) return ESR_E_ARG;
    if (map->mode != ESR_DATA_MAP_RGB && map->mode != ESR_DATA_MAP_MIX) return ESR_E_ARG;
    if (map->mode == ESR_DATA_MAP_MIX && !(map->scale > 0.0)) return ESR_E_ARG;
    const bool mixing = map->mode == ESR_DATA_MAP_MIX;
    const int lh = ph / sf, lw = pw / sf;
    int Co = 0;
    bool synth = false;
    for (int i = 0; i < B; ++i) {
        const esr_data_item& it = items[i];
        if (!it.hr || (it.channels != 1 && it.channels != 3) || it.H < 1 || it.W < 1 || it.stride < it.W) return ESR_E_ARG;
        if (it.y0 < 0 || it.x0 < 0 || it.y0 % sf || it.x0 % sf || (long long)it.y0 + ph > it.H || (long long)it.x0 + pw > it.W) return ESR_E_ARG;
        if (it.flags & ~(ESR_DATA_HFLIP | ESR_DATA_VFLIP | ESR_DATA_TRANSPOSE)) return ESR_E_ARG;
        if ((it.flags & ESR_DATA_TRANSPOSE) && ph != pw) return ESR_E_ARG;
        if (it.lr) {
            if (it.lr_H < 1 || it.lr_W < 1 || it.lr_stride < it.lr_W || it.y0 / sf + lh > it.lr_H || it.x0 / sf + lw > it.lr_W) return ESR_E_ARG;
        } else {
            synth = true;
        }
        const int co = mixing ? 1 : it.channels;
        if (Co && co != Co) return ESR_E_ARG;                 // one batch, one channel count
        Co = co;
    }
    if (synth && !taps) return ESR_E_ARG;
    DataPlan p;
    if (!data_plan(sf, k, pre, p)) return ESR_E_UNSUPPORTED;
    const long long tiles_y = (lh + p.tile - 1) / p.tile, tiles_x = (lw + p.tile - 1) / p.tile;
    if (tiles_y * tiles_x > 0x7FFFFFFFll || B > 65535) return ESR_E_UNSUPPORTED;
    const size_t lds = ((size_t)p.win * p.win * (mixing ? 4 : Co) + 15) & ~(size_t)15;
    const Mix m{map->w[0], map->w[1], map->w[2], map->b, map->scale};
    const dim3 grid((unsigned)(tiles_y * tiles_x), (unsigned)B);
    ESR_CLEAR_ERR();
    if (mixing)
        hipLaunchKernelGGL(lrhr_batch_kernel<true>, grid, dim3(DT_THREADS), lds, (hipStream_t)stream, items_dev, p, (int)tiles_x, sf, k, pre, taps, ph, pw, Co,
                           m, hr, lr);
    else
        hipLaunchKernelGGL(lrhr_batch_kernel<false>, grid, dim3(DT_THREADS), lds, (hipStream_t)stream, items_dev, p, (int)tiles_x, sf, k, pre, taps, ph, pw, Co,
                           m, hr, lr);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}
