/*
 * esr_hip.h — C-ABI of libesr_hip.so: the MI355X (gfx950) kernels behind the reference's
 * RRDB generator + Consistency Enforcing Module (CEM) hot path.
 *
 * The reference (YuvalBahat/Explorable-Super-Resolution) is pure Python/PyTorch and has no FFI of
 * its own; the operators it reaches through torch.nn are listed next to each entry point, with
 * the reference file:line they replace.  A maintainer binds these with ctypes;
 * the in-tree binding is explorable-super-resolution_amd/esr_hip/_lib.py.
 *
 * Conventions
 *   - plain C: pointers + sizes only; every pointer is a caller-owned DEVICE pointer unless it is a
 *     descriptor struct (host memory, read during the call).
 *   - return 0 on success, <0 on bad argument / unsupported shape (ESR_E_*); never throws, never
 *     allocates device memory, never synchronises the stream: work is enqueued on `stream`
 *     (hipStream_t).  Two entry points copy a HOST descriptor table to the device
 *     (esr_pack_batch_upload, esr_conv3x3_wgrad_batch[_upload]): pageable memory, staged by the
 *     runtime before the call returns — host-blocking for the duration of that staging and not
 *     capturable in a HIP graph; their *_run counterparts have no host traffic.
 *   - stateless and thread-safe: one process per GPU or several host threads may call concurrently.
 *
 * Internal activation layout ("act view"), used between the conv kernels so that dense-block
 * concatenation is zero-copy and every MFMA operand fragment is one aligned 16-byte read:
 *     [B][CG][H+2][W+2][8]  of bf16, i.e. channels in groups of 8 ("cg"), one 16-byte vector per
 *     pixel per group, with a ONE-PIXEL ZERO BORDER stored in memory (conv zero padding costs no
 *     bounds logic; producers never write the border).
 *   `hi` holds bf16(x); `lo` (optional) holds bf16(x - hi): together ~16 mantissa bits.  With both
 *   planes the conv kernels evaluate hi*hi + hi*lo + lo*hi on the bf16 MFMA pipe with fp32
 *   accumulation ("split-bf16", rel. error ~1e-5 vs fp32); with lo == NULL they run plain bf16.
 */
#ifndef ESR_HIP_H
#define ESR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESR_OK 0
#define ESR_E_ARG (-1)        /* NULL / inconsistent argument */
#define ESR_E_UNSUPPORTED (-2) /* shape outside what the kernels implement */
#define ESR_E_LAUNCH (-3)      /* HIP reported a launch error */
#define ESR_E_DATA (-4)        /* the bytes given are not what they claim to be (esr_jpeg_file_*: a truncated or corrupt file) */

typedef void* esr_stream_t;   /* hipStream_t */

/* Element formats of an activation view.  BF16 with a `lo` plane is the fp32-class mode (split operands, 3 MFMAs per product);
 * BF16 / F16 without `lo` are the single-MFMA reduced-precision modes; F16 with `lo` is the 2-MFMA mode (f16 weights x f16 hi+lo
 * activations).  The reference has no counterpart of these; the F16 modes are inference-only (gradients would need loss scaling).
 * Weight packs use the matching code in their `split` argument: 0 bf16, 1 split bf16 (hi+lo), 2 f16 (one plane), 3 f16 hi+lo. */
#define ESR_FMT_BF16 0
#define ESR_FMT_F16 1

/* A view of `ncg` consecutive channel groups inside an activation buffer. */
typedef struct {
    void* hi;                /* 16-bit planes (bf16 or fp16, see fmt), NULL = view absent */
    void* lo;                /* residual planes (value = hi + lo) or NULL: single-plane view */
    int32_t ncg;             /* number of 8-channel groups in this view */
    int32_t H, W;            /* interior size; the buffer holds (H+2) x (W+2) pixels per group */
    int64_t batch_stride;    /* in 16-byte pixel vectors */
    int64_t cg_stride;       /* in 16-byte pixel vectors (normally (H+2)*(W+2)) */
    int32_t fmt;             /* element format of the planes: ESR_FMT_BF16 (default) or ESR_FMT_F16; both as hi [+ lo] */
} esr_act_view;

/* ---- conv3x3 (+bias, +LeakyReLU, +scaled residuals, + fused nearest upsample of the input) ----
 * Replaces, per call, the reference chain
 *     torch.cat(inputs) -> nn.Conv2d(k=3,s=1,p=1,bias) -> LeakyReLU(0.2) -> .mul(0.2) + residual
 *   codes/models/modules/block.py:129-146 (conv_block), :230-235 (ResidualDenseBlock_5C.forward),
 *   :262-270 (RRDB.forward), :85-97 (ShortcutBlock.forward), :293-309 (Upsampler + upconv_blcok),
 *   codes/models/modules/architecture.py:288-301 (latent re-concatenation before every conv).
 * Also used as the data-gradient of the same conv (weights packed transposed+flipped).
 *
 *   out = alpha * act(conv(in0 ++ in1) + bias) + beta1*res1 + beta2*res2
 *
 * Limits checked by the entry point (ESR_E_ARG / ESR_E_UNSUPPORTED otherwise): 0 <= act_slope <= 1 and alpha >= 0 (the epilogue evaluates
 * alpha * LeakyReLU(y) as max(alpha*y, alpha*act_slope*y); act_slope = 0 is ReLU, torchvision VGG's nn.ReLU(inplace=True)); H + 2 and W + 2 below 32768; upsample
 * 0 or 1 (none), 2, 3, 4, 6 or 8 (ESR_E_UNSUPPORTED otherwise, checked before anything touches the device: the kernel maps an output coordinate to its
 * source by a multiplication that is exact for these factors only); every view's image (ncg * cg_stride * 16
 * bytes) and the fp32 destination's image below 4 GiB (per-lane addresses are a uniform per-image base + a 32-bit offset); res1 / res2 cover
 * every output group (ncg * 8 >= cout); mask_src covers the masked groups.
 * Epilogues with a kernel (ESR_E_UNSUPPORTED otherwise): plain; res1; res1 + res2; out_nchw; out2; mask_src; res1 + mask_src (bf16 formats only);
 * pixel_shuffle — res2 only together with res1, and out2, out_nchw, mask_src and pixel_shuffle each on its own (besides res1 + mask_src).
 * Without pixel_shuffle, an act-layout `out` (and out2) is written at the interior pixels of groups [0, ceil(cout / 8)) only: never its border, never a group behind them.  The
 * channels past cout of a partial last group are written too, with a zero conv and bias: beta1*res1 + beta2*res2 of those channels, masked like
 * the rest (zero when the residuals hold zero there).
 *
 * When res1 is a channel-group slice of in1 itself (same strides; the RDB's  conv5*0.2 + x, block.py:235) and act_slope == 1,
 * the library notices it from the pointers and takes the residual from the input tile it stages on chip anyway (no extra reads);
 * the result is the same expression evaluated in fp32.
 */
typedef struct {
    esr_act_view in0;        /* optional leading segment (latent Z group); ncg = 0 when absent */
    esr_act_view in1;        /* main segment; with upsample>1 it is read as in1[y/upsample][x/upsample] */
    int32_t upsample;        /* 0 or 1: none; 2, 3, 4, 6 or 8 (the limits above) */
    const void* wpack;       /* weights packed by esr_pack_conv_weights for (in0.ncg + in1.ncg) groups */
    const float* bias;       /* [mtiles*32] fp32, zero padded; NULL = no bias */
    int32_t cout;            /* real output channels: <= 64, or a multiple of 64 — then the launch covers cout/64 output slices at once and `wpack`
                              * holds one 64-row pack per slice, slice s at byte offset s * esr_conv_wpack_bytes(in0.ncg + in1.ncg, 64, fmt)
                              * (no out_nchw / pixel_shuffle with slices) */
    int32_t B, H, W;         /* output interior size (= input size * upsample) */
    float act_slope;         /* 1.0f: identity; 0.2f: LeakyReLU(0.2); 0.0f: ReLU */
    float alpha;
    esr_act_view res1; float beta1;   /* optional (hi == NULL: absent); same H, W as the output */
    esr_act_view res2; float beta2;
    esr_act_view out;        /* act-layout destination (ncg*8 >= cout), or hi == NULL */
    esr_act_view out2;       /* optional second destination (same values; may be hi-only when `out` is hi+lo: a one-plane copy) */
    float* out_nchw;         /* optional fp32 [B][cout][H][W] destination */
    /* data-gradient helper: multiply the result for output groups [mask_cg0, mask_cg1) by
     * act'(mask_src) = (mask_src > 0 ? 1 : mask_slope) AFTER the residual add (LeakyReLU backward of
     * the layer that produced those channels; block.py:18; mask_slope = 0: ReLU backward, the gradient passes where the stored output
     * is > 0, as torch's in-place ReLU). mask_src.hi == NULL: disabled.  Group 0 of mask_src is output group mask_cg0; only the sign of its
     * hi plane is read, in either element format.  With output slices the window is in absolute groups and may span slices. */
    esr_act_view mask_src; int32_t mask_cg0, mask_cg1; float mask_slope;
    /* scheduling hint, no effect on the result: walk the tiles (and so the images) last to first.  Consecutive layers of a network
     * re-read what the previous launch just touched; alternating the direction lets the tail of one launch, still in the 256 MB
     * Infinity Cache, be the head of the next. */
    int32_t reverse_order;
    /* planes of the weight pack: 0 = the format's default (bf16: as many as the activations; f16: one), or 1 / 2 explicitly.
     * f16 hi+lo activations with 2 weight planes is the 3-MFMA fp16 form (2^-22 operands) used for the few layers whose weight
     * rounding dominates the output error; with 1 plane it is the 2-MFMA form. */
    int32_t weight_planes;
    /* fp16 formats only: number of LEADING channel groups of in1 whose lo plane carries data (0 = all of them).  The groups behind
     * them are single-plane intermediates (a dense block's conv outputs, consumed only inside the block, where 11 bits suffice): their
     * lo plane is neither read nor multiplied — counted in K chunks of two groups, in0's included: when in0.ncg + in1_lo_groups is odd, the
     * lo plane of the first group behind them is multiplied too and must hold zero (or that group's residue).  < 0: no lo plane is multiplied.
     * Likewise `out.lo == NULL` with hi+lo inputs stores the result as one fp16 plane. */
    int32_t in1_lo_groups;
    /* pixel-shuffle store (codes/models/modules/block.py:278-291: conv to out_nc*r^2 channels, nn.PixelShuffle(r), act): with
     * pixel_shuffle = r > 1 the launch's output rows are taken in groups of 8 ("row groups"); row group g = ps_rowgroup0 + (row / 8)
     * holds the 8 channels of output group g / r^2 at sub-position s = g % r^2, and is stored to out[group][r*y + s / r][r*x + s % r]
     * (out.H == r*H, out.W == r*W).  The caller packs the weights with the matching row map: row -> conv channel
     * ((g / r^2)*8 + row % 8) * r^2 + s.  The activation commutes with the shuffle and is applied before it.  0: plain store. */
    int32_t pixel_shuffle;
    int32_t ps_rowgroup0;
    /* structurally sparse weights, a HINT: 9-bit tap masks (bit 3*dy + dx of the tap as the pack stores it; 0 = all nine taps).  The caller
     * promises that K chunk cp (the cp-th PAIR of input channel groups) has non-zero weights only at the taps of
     * tap_mask_k[(cp >> tap_mask_k_shift) & 3], and the j-th 32-row tile of the output (j = 2 * slice + tile) only at those of
     * tap_mask_m[j & 3]; the library skips blocks outside the masks where it has a kernel for the pattern and multiplies the zeros
     * otherwise — same result.  Patterns with kernels: the critic's 4x4 stride-2 convs (codes/models/modules/architecture.py:452-480) run as
     * 3x3 convs over the space-to-depth input, 16 non-zero blocks of 36 (esr_hip/critic.py): forward (K masks {432, 216, 54, 27}, shift 1) and
     * data gradient (M masks {27, 54, 216, 432}); plain epilogue, bf16 formats, cout a multiple of 64. */
    int32_t tap_mask_k[4];
    int32_t tap_mask_k_shift;
    int32_t tap_mask_m[4];
    /* optional split-K workspace (caller-owned device memory, `k_split_ws_floats` floats; NULL: never split).  A launch of few output tiles
     * with a long K axis (the critic's 256- / 512-channel layers on 16x16 ... 4x4 maps: 24-100 workgroups x 32-128 K chunks on 256 CUs) may be
     * run as S = 2, 4 or 8 sets of workgroups that each contract 1/S of the input channels into an fp32 slab of B*cout*H*W floats, followed by a
     * second launch that adds the slabs in a fixed order and stores `out`.  The library decides from its tiling (S * workgroups within the small-launch bound, 320; >= 8 chunks
     * per set, S slabs fit); only plain launches qualify (act_slope 1, no residual / mask / out2 / out_nchw / pixel_shuffle / upsample / in0,
     * bf16 formats, cout a multiple of 64).  The result differs from the unsplit launch by fp32 summation order only. */
    float* k_split_ws;
    int64_t k_split_ws_floats;
    /* scheduling hint, no effect on the result: 0 = the library picks the form by launch size (launches with no more workgroups than CUs
     * pipeline their own LDS-DMA through two stages, larger ones run two single-stage workgroups per CU); 1 / 2 = force that form. */
    int32_t lds_stages;
    /* fp16 formats only, optional (NULL: off): range watch.  The reference computes in fp32 (codes/models/modules/block.py:230-235) and has no
     * magnitude cliff; an fp16 activation plane saturates at 65504.  When a value the launch stores has magnitude >= 32768 (one binade of head
     * room left) or is not finite, the kernel does atomicMin(*range_flag, range_tag) — no extra pass, nothing on the path of a launch that stays
     * in range.  The caller initialises the word to 0xFFFFFFFF, gives every launch of a pass its own tag (its index) and reads the word when it
     * consumes the pass's result: the smallest tag names the first layer that left the range. */
    uint32_t* range_flag;
    uint32_t range_tag;
    /* the conv behind a nearest x2 upsample (codes/models/modules/block.py:293-309) as four 4-tap convs on the INPUT grid, in place of
     * upsample = 2: every 2x2 block of the upsampled image holds one value, so output phase (py, px) of out[2y + py][2x + px] reads only the 2x2
     * source neighbourhood (y - 1 + py .. y + py, x - 1 + px .. x + px), with weights that are sums of the original taps — 4/9 of the products.
     * upsample_phases = 2: H, W and in1 are the SOURCE size, out.H == 2 * H and out.W == 2 * W (ESR_E_ARG otherwise, and with upsample > 1);
     * `wpack` holds the folded packs of esr_pack_conv_weights (transposed = ESR_PACK_FOLD2 + p0): for every 32-channel block c of the output two
     * 64-row packs back to back, slice 2c (phases 0, 1: p0 = 0) and slice 2c + 1 (phases 2, 3: p0 = 2), both M tiles of a slice mapping the rows of
     * block c, slice s at byte offset s * esr_conv_wpack_bytes(in1.ncg, 64, fmt); `bias` has ceil(cout / 32) * 32 floats, indexed by channel.
     * The 32-row tile j = 2 * slice + tile of the launch is phase j & 3 of channels 32 * (j >> 2) ..., the order tap_mask_m = {27, 54, 216, 432}
     * describes; only the four live taps' weight fragments are copied and multiplied.  Epilogue: bias and alpha * LeakyReLU; one launch, a whole
     * 16-byte pixel vector per lane and group as in the plain store; the source's stored zero border is the upsampled image's zero padding.
     * Accepted: every element format (bf16, split bf16, f16, f16 hi+lo with 1 or 2 weight planes), any cout with out.ncg * 8 >= cout, both LDS
     * forms (lds_stages).  Refused with ESR_E_UNSUPPORTED: in0, res1, res2, mask_src, out2, out_nchw, pixel_shuffle, partial lo planes
     * (in1_lo_groups != 0, out.lo == NULL with hi+lo inputs), any other value than 0 or 2; tap masks and k_split_ws are ignored.  NOT checked,
     * because a pack carries no mark of how it was made: that `wpack` is the folded pack in this slice order with the planes weight_planes
     * says — a plain pack passed here is multiplied as if it were folded and the launch returns ESR_OK with a wrong result.  The result
     * differs from the upsample = 2 launch by the fp32 rounding of the folded weights (at most three additions per weight) and the shorter sum. */
    int32_t upsample_phases;
} esr_conv3x3_desc;

int esr_conv3x3(const esr_conv3x3_desc* d, esr_stream_t stream);

/* Host-only query (no device access, nothing launched): how esr_conv3x3 would tile the launch `d` describes, without split K.
 * tiling[0] / [1] = output tiles per image along x / y, [2] = M tiles (32 output channels) per workgroup, [3] = output slices (grid y; 2 when a
 * 64-channel layer of a small launch runs as two 32-channel slices; 2 * ceil(cout / 32) with upsample_phases = 2, whose tiles lie on the source grid).  The launch has tiling[0] * tiling[1] * B * tiling[3] workgroups; up to
 * 320 of them (CONV_SMALL_WGS in esr_conv.hip, the one small-launch bound) take the small-launch (multi-stage) form.  Checks only the sizes it needs (ESR_E_ARG / ESR_E_UNSUPPORTED otherwise). */
int esr_conv3x3_tiling(const esr_conv3x3_desc* d, int32_t* tiling);

/* Adjoint of the pixel-shuffle store: dst[b][g*r^2 + s][y][x] = src[b][g][r*y + s / r][r*x + s % r] for every group g of `src`
 * (dst.ncg == src.ncg * r^2, src.H == r*dst.H): the gradient of the shuffled tensor laid out in the conv's row-group order
 * (autograd of nn.PixelShuffle, block.py:287). */
int esr_pixel_unshuffle(const esr_act_view* src, int r, const esr_act_view* dst, int B, esr_stream_t stream);

/* Packed-weight size in bytes for `ncg_in` input groups and `cout` output channels
 * (`split` = 1: bf16 hi+lo planes; 0: bf16 hi only; 2: f16, one plane; 3: f16 hi+lo planes). */
size_t esr_conv_wpack_bytes(int ncg_in, int cout, int split);

/* Pack nn.Conv2d weights [cout_w][cin_w][3][3] (fp32, device) into MFMA fragment order.
 *   kmap[ncg_in*8]  : for each (group, lane-in-group) the index into the tensor's "K" channel axis, or -1 (zero)
 *   mmap[mtiles*32] : for each output row the index into the "M" channel axis, or -1 (zero)
 *   transposed = 0 : forward     — M axis = dim 0 (cout_w), K axis = dim 1 (cin_w), tap (dy,dx) as stored
 *   transposed = 1 : data-grad   — M axis = dim 1 (cin_w),  K axis = dim 0 (cout_w), tap flipped (2-dy,2-dx)
 *   transposed = ESR_PACK_FOLD2 + p0 (p0 = 0..3) : forward orientation, folded for esr_conv3x3_desc.upsample_phases = 2.  M tile m of the pack holds
 *                    phase p = (p0 + m) & 3, (py, px) = (p >> 1, p & 1): at tap position (ty, tx) of the 3x3 window over the source grid the fp32
 *                    sum of the original taps that read that source pixel — rows {0} and {1, 2} at ty = 0, 1 for py = 0, {0, 1} and {2} at
 *                    ty = 1, 2 for py = 1, columns alike; row sums first (lower index first), then the two column terms — and zero at the five
 *                    positions outside the phase's 2x2 block (tap masks 27, 54, 216, 432 for p = 0..3).  The sum is then scaled and split as
 *                    any other weight.  Other values: ESR_E_ARG.  (esr_pack_desc.transposed takes the same codes.)
 * kmap/mmap are device int32 arrays; every weight is multiplied by `scale` before it is split.
 * The pack is chunk-major ([pair of K groups][tap][mtile][hi|lo][lane]): the K axis of one launch may concatenate several tensors
 * by packing each at byte offset  first_group/2 * esr_conv_wpack_bytes(2, mtiles*32, split)  of one buffer (first_group even) —
 * how the dense-block data gradient sums  W_5^T*dy_5 + ... + W_j^T*dy_j  in a single conv (block.py:230-235 backwards). */
#define ESR_PACK_FOLD2 2
int esr_pack_conv_weights(const float* w, int cout_w, int cin_w, const int32_t* kmap, int ncg_in,
                          const int32_t* mmap, int mtiles, int transposed, int split, float scale, void* wpack,
                          esr_stream_t stream);

/* The same for MANY tensors in one launch (a training step changes every layer's weights).  `descs` is a HOST array; upload once
 * into caller-owned device `workspace` (>= esr_pack_batch_workspace_bytes), then esr_pack_batch_run re-packs all of them from the
 * CURRENT contents of their `w` whenever the parameters changed — no host traffic in steady state.  upload returns the number of
 * workgroups to pass to run (> 0), or ESR_E_*; it must be repeated when any pointer in the descriptors changes. */
typedef struct {
    const float* w; int32_t cout_w, cin_w; const int32_t* kmap; int32_t ncg_in; const int32_t* mmap;
    int32_t mtiles, transposed, split; float scale; void* wpack;
} esr_pack_desc;
int64_t esr_pack_batch_workspace_bytes(const esr_pack_desc* descs, int n);
int64_t esr_pack_batch_upload(const esr_pack_desc* descs, int n, void* workspace, int64_t workspace_bytes, esr_stream_t stream);
int esr_pack_batch_run(const void* workspace, int n, int64_t nblocks, esr_stream_t stream);

/* ---- layout conversion at the module boundary ----
 * fp32 NCHW -> act view.  Writes channels [c0, c0+nc) of `src` ([B][C][h][w]; image b starts at
 * src + b*src_batch_stride floats, 0 = C*h*w — lets the HR-resolution latent be read through the raw
 * `view` the reference applies to it, SRRaGAN_model.py:233 / architecture.py:283) into group 0.. of `dst`, with
 *   pad  : replicate padding by `pad` pixels on every side (CEM_PyTorch.forward eval-mode LR_padder /
 *          HR_padder, codes/CEM/CEMnet.py:286-295), dst interior = (h+2*pad)/down x (w+2*pad)/down
 *   down : 1, or the bilinear /down of architecture.py:284 (F.interpolate(scale_factor=1/sf,'bilinear',
 *          align_corners=False)) applied AFTER the padding (down divides h+2*pad): source coordinate
 *          max((y + 0.5)*down - 0.5, 0), taps (y0, min(y0 + 1, h + 2*pad - 1)), the same along x.
 * What is written: every vector of the (H+2) x (W+2) frame of EVERY group of dst->ncg, both planes of a two-plane view, for B images and
 * nothing else.  Stored element = hi: the value rounded to nearest even in dst->fmt, lo: the fp32 residual value - hi rounded the same way.
 * The 1-px border, the lanes >= nc of the last group and whole groups past ceil(nc / 8) are zero.  Channels of src outside [c0, c0+nc)
 * and the floats between two images (src_batch_stride > C*h*w) are not read.
 * ESR_E_ARG, before anything is launched: NULL src / dst / dst->hi; B <= 0; nc <= 0; c0 < 0; c0 + nc > C; pad < 0; down < 1; h < 1 or
 * w < 1; down not dividing h + 2*pad or w + 2*pad; dst->H, dst->W other than the interior size above; dst->ncg * 8 < nc. */
int esr_pack_nchw(const float* src, int64_t src_batch_stride, int B, int C, int h, int w, int c0, int nc, int pad, int down,
                  const esr_act_view* dst, esr_stream_t stream);
/* act view -> fp32 NCHW [B][nc][H][W] (hi + lo as one fp32 addition, an absent lo counting as +0); used by tests and by callers that want
 * features.  Reads the interior of groups 0 .. ceil(nc / 8) - 1 only; lanes >= nc of the last group go nowhere.
 * ESR_E_ARG, before anything is launched: NULL src / src->hi / dst; B <= 0; nc <= 0; src->ncg * 8 < nc; src->H < 1 or src->W < 1. */
int esr_unpack_nchw(const esr_act_view* src, int B, int nc, float* dst, esr_stream_t stream);
/* zero `n16` 16-byte vectors (border initialisation of freshly allocated activation buffers); n16 == 0 is ESR_OK and launches nothing,
 * p == NULL or n16 < 0 ESR_E_ARG */
int esr_zero(void* p, int64_t n16, esr_stream_t stream);

/* ---- VGG feature extractor glue (the perceptual loss's network: codes/models/modules/architecture.py:658-705, VGGFeatureExtractor on
 * torchvision's VGG `features` = Conv2d(3x3, pad 1) / ReLU(inplace) / MaxPool2d(2, 2) layers; the convs and their ReLU are esr_conv3x3
 * launches with act_slope = 0, their data gradients esr_conv3x3 on transposed packs with mask_slope = 0).
 * esr_pack_nchw_norm: fp32 NCHW [B][C][h][w] -> act view (h x w, zero border) of (x - mean[c]) / std[c] — VGGFeatureExtractor.forward's
 *   input normalisation (architecture.py:705-709) applied BEFORE conv1_1's zero padding, so the border stays 0.  mean / std: device fp32 [C],
 *   both NULL = no normalisation (use_input_norm = False).  As esr_pack_nchw, every group of dst->ncg is written whole: the border, the
 *   lanes >= C and the groups past ceil(C / 8) are zero (not (0 - mean) / std).  ESR_E_ARG: a NULL src / dst / dst->hi; B, C, h or w <= 0;
 *   one of mean / std without the other; dst->H != h or dst->W != w; dst->ncg * 8 < C.
 * esr_unpack_grad_nchw_norm: its adjoint — act-layout gradient (hi + lo) -> fp32 NCHW [B][C][G->H][G->W], divided by std[c] (NULL: copied).
 *   Groups past ceil(C / 8) are not read; lanes >= C of the last group go nowhere.  ESR_E_ARG: a NULL G / G->hi / dst; B or C <= 0; G->ncg * 8 < C; G->H or G->W <= 0.
 * esr_maxpool2x2: nn.MaxPool2d(kernel_size=2, stride=2) — y->H = floor(x->H / 2), y->W = floor(x->W / 2) (F.max_pool2d floors); the window
 *   value is hi + lo; the output is the element at torch's argmax (the first maximum in row-major window order; a NaN propagates), copied
 *   bit for bit, and y's one-pixel zero border is written (y is the next conv's input).  Same format and planes in x and y.
 * esr_maxpool2x2_grad: its backward — dx (x's size, zero border written, as are the uncovered last row / column of odd sizes) receives dy
 *   at the argmax of every window, recomputed from the saved pre-pool x, and zero elsewhere; relu_mask != 0 also zeroes it where x <= 0
 *   (x is a ReLU's output: the ReLU's backward, fused).  dy and dx share format and planes; x may have either. */
int esr_pack_nchw_norm(const float* src, int B, int C, int h, int w, const float* mean, const float* std, const esr_act_view* dst, esr_stream_t stream);
int esr_unpack_grad_nchw_norm(const esr_act_view* G, int B, int C, const float* std, float* dst, esr_stream_t stream);
int esr_maxpool2x2(const esr_act_view* x, const esr_act_view* y, int B, esr_stream_t stream);
int esr_maxpool2x2_grad(const esr_act_view* x, const esr_act_view* dy, int relu_mask, const esr_act_view* dx, int B, esr_stream_t stream);

/* ---- Consistency Enforcing Module filters (fixed depth-wise taps, fp32, NCHW) ----
 * codes/CEM/CEMnet.py:243-252 (Filter_Layer) x3 as built in CEM_PyTorch.__init__ (:254-281).
 * `taps` are device fp32 [k][k] arrays exactly as the reference stores them in Filter_OP.weight[0,0]. */

/* DownscaleOP (CEMnet.py:272-275): replicate-pad floor(k/2), correlate with taps (= rot90(ds_kernel,2)),
 * keep [pre::sf, pre::sf].  y: [B][C][sf*h][sf*w] -> d: [B][C][h][w].
 * If lr != NULL the kernel writes  lr_pad - d  instead, where lr_pad is `lr` ([B][C][h-2*lr_pad][w-2*lr_pad])
 * replicate-padded by lr_pad (fuses the LR_padder and the x - D(g) of the projection). */
int esr_cem_downscale(const float* y, int B, int C, int h, int w, int sf, int pre, const float* taps, int k,
                      const float* lr, int lr_pad, float* d, esr_stream_t stream);
/* Conv_LR_with_Inv_hTh_OP (CEMnet.py:261-263): replicate-pad floor(k/2), correlate. [B][C][h][w] -> same. */
int esr_cem_lrfilter(const float* x, int B, int C, int h, int w, const float* taps, int k, float* out,
                     esr_stream_t stream);
/* Upscale_OP (CEMnet.py:264-271): zero-stuff at (pre,pre), replicate-pad floor(k/2), correlate with taps
 * (= ds_kernel*sf^2), any pre in [0, sf): the padding repeats the first row / column of the zero-stuffed image — samples
 * when pre == 0 — and the last — samples when pre == sf-1 — and holds zeros otherwise.
 * f: [B][C][h][w] -> [B][C][sf*h][sf*w], restricted to the crop window
 * [crop, sf*h-crop) x [crop, sf*w-crop) (HR_unpadder, CEMnet.py:311).
 *   mode 0: out = U(f)
 *   mode 1: out = g + U(f)                      (projection  g + U(K(x - D(g))), CEMnet.py:305-310)
 *   mode 2: out = U(f_x) + tanh(g - U(f_g)) * range      (sigmoid_range_limit; f = f_x, f2 = f_g)
 *   mode 3: out = U(f_x), out2 = g - U(f_g)              (decomposed_output)
 * g/out/out2 are [B][C][sf*h][sf*w] and [B][C][sf*h-2crop][sf*w-2crop] respectively. */
int esr_cem_upscale(const float* f, const float* f2, int B, int C, int h, int w, int sf, int pre,
                    const float* taps, int k, const float* g, int crop, int mode, float range,
                    float* out, float* out2, esr_stream_t stream);

/* The three filters above with ONE TAP SET PER IMAGE: `taps` is a device fp32 [B][k][k] array, image b's C planes all use taps[b] (a batch whose
 * images were blurred by different kernels — estimated ones are not rank one, hence the 2-D forms only).  Every other argument, the index conventions,
 * the fused forms (lr / lr_pad; modes 0..3, crop, range, out2), the kernel forms (LDS-tiled where the window fits and B * C <= 65535, else one output
 * per thread) and the error codes are those of esr_cem_downscale / esr_cem_lrfilter / esr_cem_upscale; with B equal tap sets the results are theirs
 * bit for bit.  Forward only: there is no per-image adjoint. */
int esr_cem_downscale_per_image(const float* y, int B, int C, int h, int w, int sf, int pre, const float* taps, int k,
                                const float* lr, int lr_pad, float* d, esr_stream_t stream);
int esr_cem_lrfilter_per_image(const float* x, int B, int C, int h, int w, const float* taps, int k, float* out,
                               esr_stream_t stream);
int esr_cem_upscale_per_image(const float* f, const float* f2, int B, int C, int h, int w, int sf, int pre,
                              const float* taps, int k, const float* g, int crop, int mode, float range,
                              float* out, float* out2, esr_stream_t stream);

/* Separable variants of the three CEM filters for rank-one taps  taps[a][b] = tv[a] * th[b]  (the bicubic ds_kernel and its inv_hTh are
 * rank one; estimated / anisotropic kernels are not and use the 2-D entry points): a horizontal and a vertical 1-D pass on the tile a
 * workgroup holds on chip, 2k instead of k^2 MACs per output.  Arguments, index conventions, fused forms and results as esr_cem_downscale /
 * esr_cem_lrfilter / esr_cem_upscale (up to fp32 rounding of the tap products); `tv`, `th`: device arrays of k floats.
 * ESR_E_UNSUPPORTED: the tile does not fit on chip for this (sf, k) — use the 2-D entry point. */
int esr_cem_downscale_sep(const float* y, int B, int C, int h, int w, int sf, int pre, const float* tv, const float* th, int k, const float* lr,
                          int lr_pad, float* d, esr_stream_t stream);
int esr_cem_lrfilter_sep(const float* x, int B, int C, int h, int w, const float* tv, const float* th, int k, float* out, esr_stream_t stream);
int esr_cem_upscale_sep(const float* f, const float* f2, int B, int C, int h, int w, int sf, int pre, const float* tv, const float* th, int k,
                        const float* g, int crop, int mode, float range, float* out, float* out2, esr_stream_t stream);
/* esr_cem_lrfilter_sep followed by esr_cem_upscale_sep as ONE launch: every mode of esr_cem_upscale_sep with K(e) (and K(e2)) in place of f (f2),
 * K = the kf-tap separable LR filter tvf x thf with replicate padding (CEM_PyTorch.forward's Conv_LR_with_Inv_hTh_OP in front of Upscale_OP,
 * codes/CEM/CEMnet.py:305-309).  Each tile filters its own window of e on chip, with the separate kernel's passes and summation order: results are
 * bit-identical to the two launches, the LR-sized intermediate and its launch are gone.  ESR_E_UNSUPPORTED: the windows do not fit on chip for this
 * (sf, k, kf) — run the two launches. */
int esr_cem_filter_upscale_sep(const float* e, const float* e2, int B, int C, int h, int w, int sf, int pre, const float* tvf, const float* thf, int kf,
                               const float* tv, const float* th, int k, const float* g, int crop, int mode, float range, float* out, float* out2,
                               esr_stream_t stream);

/* Which kernel form esr_cem_downscale_sep (op 0) / esr_cem_upscale_sep (op 1) / esr_cem_lrfilter_sep (op 2; k = its tap count, sf and pre unused) runs for an image geometry — decided from these arguments alone, never
 * from the batch, so that a batch and its chunks run the same arithmetic: 0 = tile kernel (a workgroup stages a window in LDS), 1 = streaming tile
 * kernel (x8 downscale of small images; any sf whose tile window would crowd the chip), 2 = wave-streaming kernel (low-resolution images of h * w >= 4096 pixels, sf 2 / 3 / 4 / 8 with
 * ceil(k / sf) in 4..6; the upscale: sf 3 / 4 / 8 and 0 < pre < sf - 1; the LR filter: k = 27 or 35 and h * w >= 16384 pixels): a wave walks down a strip with the vertical pass in registers.  The
 * upscale forms agree to the bit, the downscale and LR-filter forms to fp32 rounding (different order of the two passes).  For tests and documentation; < 0: ESR_E_ARG. */
int esr_cem_sep_form(int op, int sf, int k, int pre, int h, int w);

/* ---- backward-pass helpers (autograd of the reference's torch ops) ----
 * out = alpha*A + beta*sumpool_s(Bv), optionally * LeakyReLU'(mask) — gradient of the nearest upsample
 * (block.py:293-300), of residual sums, and of LeakyReLU (block.py:18).  A / Bv / mask may be NULL. */
int esr_act_combine(const esr_act_view* A, float alpha, const esr_act_view* Bv, float beta, int s, const esr_act_view* mask,
                    float mask_slope, const esr_act_view* out, int B, esr_stream_t stream);
/* Adjoint of esr_pack_nchw (replicate padding folded back onto the edge pixels, bilinear /down taps transposed):
 * act-layout gradient -> fp32 NCHW gradient of channels [c0, c0+nc) of the un-padded source. */
int esr_unpack_grad_nchw(const esr_act_view* G, float* dst, int64_t dst_batch_stride, int B, int C, int h, int w, int c0, int nc,
                         int pad, int down, int accumulate, esr_stream_t stream);
/* Magnitude management of fp16 gradients (the 'mixed' precision's backward; no counterpart in the reference, whose gradients are fp32):
 * esr_grad_absmax: *slot = max(*slot, bit pattern of max|hi|) over the view's groups (fp16 planes; the caller zeroes the slot once).
 * esr_grad_scale : dst = src * f (hi and lo planes; dst may be src), f a power of two taken from device memory:
 *   slot != NULL : f = 2^k with max|hi| * 2^k in [2^(exp-1), 2^exp)  (k = 0 when the view is all zero); scale_out, if given, receives
 *                  scale_in[0] * f — the running scale of the gradients in flight;
 *   slot == NULL : f = scale_in[0] / scale_den[0].
 * Nothing is read back by the host. */
int esr_grad_absmax(const esr_act_view* v, int B, uint32_t* slot, esr_stream_t stream);
int esr_grad_scale(const esr_act_view* src, const esr_act_view* dst, int B, const uint32_t* slot, int exp, const float* scale_in,
                   const float* scale_den, float* scale_out, esr_stream_t stream);
/* Adjoint of a CEM filter (see csrc/esr_cem.hip): y[q] = sum taps * frame[clamp(q*sq+oq + a - p)], unknowns at n*sn+on, on a frame of
 * Ny x Nx >= 1 x 1 pixels (Ny == 1 / Nx == 1: the one position takes every tap).
 * tabs: device fp32 [3][3][k][k] prefix/plain/suffix tap tables (esr_hip/cem_ops.py builds them). */
int esr_cem_adjoint(const float* dy, int B, int C, int hq, int wq, int sq, int oq, int Ny, int Nx, const float* tabs, int k,
                    int hn, int wn, int sn, int on, float* dx, int accumulate, esr_stream_t stream);
/* The same adjoint for rank-one taps (= outer(tv, th): the bicubic kernels and their inv_hTh): two 1-D passes through `tmp` (B*C*hq*wn floats).
 * tabs_v / tabs_h: device fp32 [3][k] prefix / plain / suffix sums of the vertical / horizontal factor.  dx = (base ? base : 0) + alpha * adjoint. */
int esr_cem_adjoint_sep(const float* dy, int B, int C, int hq, int wq, int sq, int oq, int Ny, int Nx, const float* tabs_v, const float* tabs_h, int k,
                        int hn, int wn, int sn, int on, float* tmp, const float* base, float alpha, float* dx, esr_stream_t stream);

/* ---- conv3x3 weight / bias gradient (autograd of nn.Conv2d, block.py:141-142) ----
 *   dw[co][lat+ci][dy][dx] += alpha * sum_{b,y,x} dy[b,co,y,x] * x[b,ci,(y+dy-1)/up,(x+dx-1)/up]     (zero padded)
 *   dw[co][e][dy][dx]      += ... with xlat for the latent channels e < lat;   db[co] += alpha * sum dy
 * dw ([cout][lat+cin_main][3][3]) and db ([cout], may be NULL) are fp32 and ACCUMULATED into (zero them first); nothing outside them is written.
 * The pixel sum is split over ~3 workgroups per CU; their partial tiles go through `workspace` (caller-owned device memory of at
 * least esr_conv3x3_wgrad_workspace_floats(d) floats, contents undefined afterwards) and a second small kernel folds them.
 * Checked by the entry point (ESR_E_ARG otherwise, before anything touches the device): dy, x, dw given; x.H * upsample == H and
 * x.W * upsample == W for ANY upsample >= 1 (0 = 1; the source coordinate is an integer division, exact for every factor); dy and xlat are
 * H x W; xlat only with upsample 1 and 1 <= lat <= 8; the views cover the channels named — dy.ncg * 8 >= cout, x.ncg * 8 >= cin_main,
 * xlat.ncg * 8 >= lat (a group past a view's end would be read as zeros); all views in one element format and all hi+lo or all hi-only.
 * fp16 hi+lo operands: ESR_E_UNSUPPORTED (fp16 runs the hi planes only).  Preconditions not checked: every view's one-pixel border is
 * zero in all 8 lanes (it is the conv's zero padding, and the reads past the image's edge land on it); lanes past cout / cin_main / lat
 * of a partial last group may hold anything, NaN included — they reach no stored element. */
typedef struct {
    esr_act_view dy;         /* gradient w.r.t. the conv's (pre-activation) output, cout channels */
    esr_act_view x;          /* the conv's main input (before the nearest upsample when upsample > 1) */
    esr_act_view xlat;       /* optional latent segment (hi == NULL: absent) */
    int32_t lat;             /* real latent channels (<= 8) */
    int32_t upsample;
    int32_t cout, cin_main;
    int32_t B, H, W;         /* output-resolution size */
    float alpha;
    float* dw;
    float* db;
    float* workspace;
    int64_t workspace_floats;
    /* a HINT, as esr_conv3x3_desc.tap_mask_k: the weights whose gradient this is are structurally zero outside the taps of tap_masks[i & 3] for
     * the i-th 32-channel tile of the main input (0 = all taps).  dw entries inside the masks, and every entry of the latent channels,
     * receive the gradient.  Entries outside them are the caller's to ignore: the one pattern with a kernel — the space-to-depth masks
     * {432, 216, 54, 27} with cin_main % 128 == 0 and bf16 operands (ESR_WGRAD_FORM_S2D) — leaves them as they were; every other case
     * (any other pattern, fp16 operands, cin_main % 128 != 0) adds the true gradient there, as without the hint. */
    int32_t tap_masks[4];
} esr_wgrad_desc;
/* Depends on everything that shapes the launch: B, H, W, cout, cin_main; xlat (given or not) and lat; upsample; the operand format and planes;
 * tap_masks (the space-to-depth tiles change the tile count, the 27-column forms the group count) — ask with the descriptor the launch will get.
 * <0: bad argument (a size <= 0; nothing else is checked here). */
int64_t esr_conv3x3_wgrad_workspace_floats(const esr_wgrad_desc* d);
int esr_conv3x3_wgrad(const esr_wgrad_desc* d, esr_stream_t stream);
/* Host-only query (no device access, nothing launched), for tests and documentation: how esr_conv3x3_wgrad runs the launch `d` describes.
 * out[0] / [1] = pixel tiles per image along x / y, [2] = tile shape (0: 8 rows x 32 columns, 1: 16 x 16, 2: 32 x 8 — the latter two only
 * with ESR_WGRAD_FORM_S2D, for the layer that has fewer tiles so), [3] = slices of the pixel sum (1: the workgroups add straight into dw / db;
 * more: partial tiles through the workspace and the fold kernel), [4] = ESR_WGRAD_FORM_* bits.  The same checks as esr_conv3x3_wgrad. */
#define ESR_WGRAD_FORM_LAT27 1       /* the latent segment (lat <= 3) runs as ONE 27-column MFMA tile (channel x tap) */
#define ESR_WGRAD_FORM_MAIN27 2      /* the main input (cin_main <= 3, no latent, no upsample) runs in that form */
#define ESR_WGRAD_FORM_S2D 4         /* the space-to-depth kernel: skips the blocks outside the masks, has the 16x16 / 32x8 tiles */
#define ESR_WGRAD_FORM_FAST_COPY 8   /* one-plane operands without upsample: tile copies from offsets computed once per workgroup */
int esr_conv3x3_wgrad_tiling(const esr_wgrad_desc* d, int32_t* out);
/* The weight gradients of MANY layers in one launch (a whole backward pass): with hundreds of layers there are enough
 * (layer, 32-input-channel tile, 32-output-channel tile) blocks to fill the chip without splitting the pixel sum, so the per-layer
 * reduction traffic and launch tails disappear.  `descs` is a HOST array (its workspace fields are ignored); `workspace` is caller-
 * owned device memory of at least esr_conv3x3_wgrad_batch_workspace_bytes(descs, n) bytes (descriptor table + partial sums).
 * All dy / x buffers must stay alive and unmodified until the launch has run; every layer must use the same operand format. */
int64_t esr_conv3x3_wgrad_batch_workspace_bytes(const esr_wgrad_desc* descs, int n);
int esr_conv3x3_wgrad_batch(const esr_wgrad_desc* descs, int n, void* workspace, int64_t workspace_bytes, esr_stream_t stream);
/* The same in two steps, for callers whose descriptor set repeats from one backward pass to the next (pooled gradient buffers, the
 * allocator handing back the same dW storage): _upload writes the descriptor table into `workspace` (a host-blocking copy from pageable
 * memory: NOT capturable in a HIP graph) and fills `plan`; _run enqueues the launch from the table already on the device (capturable; no
 * host traffic).  esr_conv3x3_wgrad_batch == _upload followed by _run. */
/* (plan fields are the library's own bookkeeping between _upload and _run — opaque to callers: nwg = workgroups of the per-pair launch, `reserved` =
 * always 0) */
typedef struct { int64_t nwg, table_bytes; int32_t n, max_red, split, f16, s2d, reserved; } esr_wgrad_batch_plan;
int esr_conv3x3_wgrad_batch_upload(const esr_wgrad_desc* descs, int n, void* workspace, int64_t workspace_bytes, esr_wgrad_batch_plan* plan,
                                   esr_stream_t stream);
int esr_conv3x3_wgrad_batch_run(const void* workspace, const esr_wgrad_batch_plan* plan, esr_stream_t stream);
/* The same launch for a SECOND stream that runs under another stream's kernels (the generator backward: weight gradients of the layers whose
 * data gradients are done, while the data-gradient chain — small launches that leave most of every CU idle — goes on): one-plane operand sets run an
 * instantiation whose waves hold more than half of a SIMD's registers, i.e. ONE workgroup per CU, so that the other stream's workgroups always find
 * room; the results are those of _run.  hi+lo / space-to-depth sets: identical to _run. */
int esr_conv3x3_wgrad_batch_run_side(const void* workspace, const esr_wgrad_batch_plan* plan, esr_stream_t stream);
/* Resident workgroups per CU of the instantiation _run_side launches for one-plane operand sets (f16: the fp16 one, else bf16), as the runtime
 * reports it for the current device (hipOccupancyMaxActiveBlocksPerMultiprocessor): 1 when the register cap holds.  The cap comes from the
 * register allocator honouring a clobber — a property of the toolchain that built the library, not of the source — so callers that schedule a
 * two-stream backward around it (esr_hip/engine.py: wgrad_overlap) ask once and keep the one-stream form when the answer is not 1.  Negative:
 * ESR_E_LAUNCH (no device / query failed).  (The reference has no counterpart: autograd's weight gradients run wherever cuDNN puts them,
 * codes/models/SRRaGAN_model.py:418-499.) */
int esr_conv3x3_wgrad_side_occupancy(int f16);
/* A backward pass's layers as SEVERAL launches (one per gradient bucket of a data-parallel job, so that each bucket's all-reduce starts behind its
 * launch and overlaps the launches that follow — torch.distributed over RCCL; the reference's nn.DataParallel reduces after the whole backward,
 * codes/models/SRRaGAN_model.py:418-499): _unit returns the slicing the ONE-launch form would use for the whole set (an opaque value: the
 * granule, and whether the set runs the 16x16 / 32x8 tiles because one of its layers is space-to-depth); passing it to _part_workspace_bytes /
 * _part_upload for every part keeps each layer's tiles and pixel sum cut exactly as in the one launch — the parts' results are bit-identical
 * to it, whichever parts hold the space-to-depth layers.  _run is the same for parts. */
int64_t esr_conv3x3_wgrad_batch_unit(const esr_wgrad_desc* descs, int n);
int64_t esr_conv3x3_wgrad_batch_part_workspace_bytes(const esr_wgrad_desc* descs, int n, int64_t unit);
int esr_conv3x3_wgrad_batch_part_upload(const esr_wgrad_desc* descs, int n, void* workspace, int64_t workspace_bytes, esr_wgrad_batch_plan* plan,
                                        int64_t unit, esr_stream_t stream);
/* Every dw / db of an uploaded table moved by the same byte offset (all layers' gradients are views of one flat buffer and the caller got a new
 * flat buffer for this pass): patch the table on the device — one tiny launch, no host traffic, stream-ordered behind the previous run. */
int esr_conv3x3_wgrad_batch_rebase(void* workspace, const esr_wgrad_batch_plan* plan, int64_t delta_bytes, esr_stream_t stream);

/* ---- Z-objective kernels (reference: codes/Z_optimization.py:170-209, SoftHistogramLoss.ComputeSoftHistogram, gray-scale / patch-size-1
 * form).  Soft histogram of n values with K bins whose centres run from lo to hi:  h[k] = (1/n) sum_i exp(-(d(v_i, c_k) + eps)^2 / T), the
 * distance wrapped with period hi as the reference does.  The forward writes one partial (un-normalised) histogram of K doubles per slab of
 * pixels — esr_soft_hist_slabs(n) of them — which the caller sums and divides by n; the backward takes d loss / d h[k] (already divided by n)
 * and writes d loss / d v.  The reference builds the n x K matrix in float64; these kernels never materialise it. */
int64_t esr_soft_hist_slabs(int64_t n);
int esr_soft_hist_fwd(const float* v, int64_t n, int K, float lo, float hi, float T, float eps, double* partial, esr_stream_t stream);
int esr_soft_hist_bwd(const float* v, int64_t n, int K, float lo, float hi, float T, float eps, const float* gh, float* gv, esr_stream_t stream);

/* ---- pairwise KDE between D-dimensional points (csrc/esr_kde.hip): the patch-histogram and dictionary Z objectives ----
 * s_ij = (1/D) sum_d (w(x_id - b_jd) + 1e-7)^2 with w the distance wrapped with period `period`, k_ij = exp(-s_ij / T); `scale` = 1 / (D T).
 * D is 1, 4, 9, 16, 25, 36, 49 or 64 (esr_kde_dim_supported).  Nothing of size N x M is stored.
 * esr_kde_fwd: for every outer point o and inner range r (ranges[2r] .. ranges[2r+1], indices into `inner`):
 *   psum[r * n_outer + o] * exp(pmax[r * n_outer + o]) = sum over the range of k_oi   (log-domain: a running max and a scaled double sum).
 * esr_kde_bwd: dxpart[s][i][d] for tiles (b, row0, row1) of at most 256 rows of one image b and bin slab s = [s * bins_per_slab, ...):
 *   sum_j g_row[i] g_bin[b][j] exp(-s_ij / T - l_row[i] - l_bin[b][j]) d(-s_ij / T)/dx_id;  g_row / l_row may be null (1 / 0), g_bin and l_bin
 *   are both null (1 / 0) or both [B][M].  The caller sums the slabs.
 * esr_kde_dedup: keep[i] = 0 iff some j > i has |b_id - b_jd| < half_width in every d (the reference's Desired_Im_2_Bins). */
int esr_kde_dim_supported(int D);
int esr_kde_fwd(const float* outer, int64_t n_outer, const float* inner, const int32_t* ranges, int n_ranges, int D, float period, float scale, float* pmax,
                double* psum, esr_stream_t stream);
int esr_kde_bwd(const float* X, int64_t R, const int32_t* tiles, int n_tiles, const float* bins, int M, int bins_per_slab, int n_slabs, int D, float period,
                float scale, const float* g_row, const float* l_row, const float* g_bin, const float* l_bin, float* dxpart, esr_stream_t stream);
int esr_kde_dedup(const float* bins, int M, int D, float half_width, int32_t* keep, esr_stream_t stream);

/* ---- Adam over many tensors in one launch ----
 * The reference steps both networks with torch.optim.Adam (codes/models/SRRaGAN_model.py:147-160: lr, betas, weight decay from the options);
 * torch's multi-tensor implementation costs ~4 ms of host time per step for the generator's 702 tensors.  Same update rule, same fp32
 * operation order (torch/optim/adam.py, no amsgrad / maximize):
 *     g += weight_decay * p;  m += (1 - beta1) * (g - m);  v = beta2 * v + (1 - beta2) * g * g;
 *     p -= (lr / bias_correction1) * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with bias_correction1 = 1 - beta1^t and bias_correction2_sqrt = sqrt(1 - beta2^t) computed by the caller for step t.
 * `tensors` is a HOST array; _upload writes it (plus a work table) into caller-owned device `workspace` (>= _workspace_bytes), blocks until
 * the copy is done and returns the chunk count to pass to _run (>= 0) or ESR_E_*; it is repeated only when a pointer changes.
 * esr_adam_table writes the same table into caller-owned HOST memory instead (>= _workspace_bytes; e.g. a pinned buffer) and returns the
 * chunk count: a caller whose gradient tensors move from step to step copies it to the device workspace itself, asynchronously on its
 * stream — no host synchronisation (the training loop of codes/train.py:90-192 has none between optimizer steps either). */
typedef struct { float* p; const float* g; float* m; float* v; int64_t n; } esr_adam_tensor;
int64_t esr_adam_workspace_bytes(const esr_adam_tensor* tensors, int n);
int64_t esr_adam_upload(const esr_adam_tensor* tensors, int n, void* workspace, int64_t workspace_bytes, esr_stream_t stream);
int64_t esr_adam_table(const esr_adam_tensor* tensors, int n, void* host_table, int64_t host_bytes);
int esr_adam_run(const void* workspace, int n, int64_t nchunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                 float bias_correction1, float bias_correction2_sqrt, esr_stream_t stream);

/* Per-image statistics of the SR output and their gradients — the reductions of the Z-search loop and of the L_struct training loss, one pass
 * over the image each (csrc/esr_zobj.hip):
 *   kind 0  masked STD       codes/Z_optimization.py:383-388  torch.std(image * mask, dim=(1,2,3))              sums[b] = (sum v, sum v^2, -)
 *   kind 1  TV_Loss          codes/Z_optimization.py:324-326                                                       sums[b] = (sum |dx|, sum |dy|, -)
 *   kind 2  structure tensor codes/models/modules/loss.py:49-62,141-151 (2x2 difference filters, (H-1) x (W-1) frame)  sums[b] = (sum ix^2, sum iy^2, sum ix iy)
 * x: fp32 [B][C][H][W]; v = clamp(x, 0, 1) when clamp01 (the reference's Output_Batch(within_0_1=True)), times mask [H][W] when given (the GUI's
 * image mask).  sums: [B][3] doubles, zeroed by the caller (the kernels add).  _grad: dx (+)= the gradient of a scalar of the three sums whose
 * chain rule the caller has folded (sqrt, division by N) into coef[b][3], the coefficients of the closed forms of csrc/esr_zobj.hip:
 *   kind 0  d/dx ( coef0/2 sums1 + coef1 sums0 )                    = (coef0 v + coef1) dv/dx
 *   kind 1  d/dx ( coef0 sums0 + coef1 sums1 )
 *   kind 2  d/dx ( coef0/2 sums0 + coef1/2 sums1 + coef2 sums2 )    (d/d ix = coef0 ix + coef2 iy, d/d iy = coef1 iy + coef2 ix)
 * with dv/dx = mask [0 <= x <= 1] as asked; accumulate != 0 adds into dx. */
int esr_img_stats(const float* x, int B, int C, int H, int W, const float* mask, int clamp01, int kind, double* sums, esr_stream_t stream);
int esr_img_stats_grad(const float* x, int B, int C, int H, int W, const float* mask, int clamp01, int kind, const float* coef, float* dx, int accumulate,
                       esr_stream_t stream);

/* ---- local-STD and periodicity Z objectives (csrc/esr_local.hip; reference codes/Z_optimization.py:459-509, 616-627, 799-815) ----
 * x: fp32 [B][C][H][W]; every kernel reads v = clamp(x, 0, 1) (channel mean for the patch STD).
 * esr_patch_std: for every corner (cy, cx) of the uint8 map corners [H-6][W-6] that is nonzero, the 7 x 7 window with that top-left corner of
 *   v = mean_c clamp(x_c, 0, 1): mean[b][cy][cx] and the unbiased std S[b][cy][cx]; unselected corners get 0.  H, W >= 7.
 * esr_patch_std_grad: dx (+)= d/dx sum_p dS[p] S[p] with dS on the same [B][H-6][W-6] grid; the terms with S = 0 contribute 0 (not NaN).
 * esr_shift_l1: one period point.  Separable bilinear samplers (grid_sample, zero padding) for the signs + (index 0) and - (index 1):
 *   base_x / frac_x [2][nx] per output column, base_y / frac_y [2][ny] per output row, weights (1 - frac, frac) on (base, base + 1).
 *   partial[b][i] = sum_{c,j} M(i,j) |GS+(v)(c,i,j) - GS-(v)(c,i,j)| (double), M = GS+(mask) GS-(mask), mask [H][W] (required).
 * esr_shift_l1_grad: dx (+)= d/dx sum_b g[b] sum_{c,i,j} M |GS+ - GS-| through work [B][C][ny][nx] (scratch); ranges_x [2][W][2] and
 *   ranges_y [2][H][2] are, per sign and source column / row, the half-open range of output columns / rows whose taps may touch it
 *   (a superset is fine: the kernel checks every tap).  Deterministic (no atomics). */
int esr_patch_std(const float* x, int B, int C, int H, int W, const uint8_t* corners, float* S, float* mean, esr_stream_t stream);
int esr_patch_std_grad(const float* x, int B, int C, int H, int W, const uint8_t* corners, const float* S, const float* mean, const float* dS, float* dx,
                       int accumulate, esr_stream_t stream);
int esr_shift_l1(const float* x, int B, int C, int H, int W, const float* mask, int nx, int ny, const int32_t* base_x, const float* frac_x,
                 const int32_t* base_y, const float* frac_y, double* partial, esr_stream_t stream);
int esr_shift_l1_grad(const float* x, int B, int C, int H, int W, const float* mask, int nx, int ny, const int32_t* base_x, const float* frac_x,
                      const int32_t* base_y, const float* frac_y, const int32_t* ranges_x, const int32_t* ranges_y, const float* g, float* work, float* dx,
                      int accumulate, esr_stream_t stream);

/* ---- scribble Z objective and its region constraint (csrc/esr_scribble.hip; reference codes/Z_optimization.py:344-364, 385-390, 401-448,
 * 743-746) ----
 * x: fp32 [B][C][H][W], read as v = clamp(x, 0, 1); desired [C][H][W] (the desired image D); labels [H][W], one byte per pixel: bit 7 the L1
 * set (image mask and 0 < scribble < 4), bit 6 the constraint set (outside the image mask), bits 0-5 a TV region id (0 = none); i0: the
 * initial output [i0_batch][C][H][W] with i0_batch 1 (broadcast) or B, or NULL (bit 6 ignored).
 * esr_scribble: partial[b][y][5] (doubles) = the row-y parts of (sum_{c,p in L1} |v - D|, the TV pair sums over d = (1,1) and (-1,1), over
 *   d = (1,0), over d = (0,1): sum_{c,p} [T(p) = T(p + d) > 0] |v(p) - v(p + d)|, and sum_{c,p in constraint} |v - I0|).  The caller sums the
 *   rows; L_b = l1 / (C H W) + tv_d / (C (H-1)(W-1)) + tv_v / (C (H-1) W) + tv_h / (C H (W-1)).
 * esr_scribble_grad: dx (+)= d/dx ( sum_b g[b] L_b + g_con sum_{b,c,p in constraint} |v - I0| ).  Deterministic (no atomics). */
int esr_scribble(const float* x, int B, int C, int H, int W, const float* desired, const uint8_t* labels, const float* i0, int i0_batch, double* partial,
                 esr_stream_t stream);
int esr_scribble_grad(const float* x, int B, int C, int H, int W, const float* desired, const uint8_t* labels, const float* i0, int i0_batch, const float* g,
                      float g_con, float* dx, int accumulate, esr_stream_t stream);

/* ---- patch-magnitude Z objective (csrc/esr_patchmag.hip; reference codes/Z_optimization.py:391-394, 450-455, 717-722) ----
 * x: fp32 [B][C][H][W], read as the gray image v = mean_c clamp(x_c, 0, 1); corner_index: int32 [H-6][W-6], the ordinal p in [0, P) of the
 * selected 7 x 7 window with that top-left corner, -1 (or anything outside [0, P)) where none is selected; desired: fp32 [P][49], one desired
 * patch per window, its pixels row-major.  H, W >= 7, P >= 1.
 * esr_patch_mag: partial[b][k] (doubles), k < esr_patch_mag_blocks(H, W): workgroup k's part of sum_p sum_{j < 49} (v(window p, j) -
 *   desired[p][j])^2; the caller sums over k and divides by 49 P.  No atomics: two calls give the same bits.
 * esr_patch_mag_grad: dx (+)= d/dx sum_b g[b] / (49 P) sum_{p, j} (v - desired)^2.  Gather form (a pixel walks the at most 49 corners whose
 *   window covers it), no atomics, deterministic; pixels under no selected window get exactly 0. */
int64_t esr_patch_mag_blocks(int H, int W);
int esr_patch_mag(const float* x, int B, int C, int H, int W, const int32_t* corner_index, const float* desired, int P, double* partial,
                  esr_stream_t stream);
int esr_patch_mag_grad(const float* x, int B, int C, int H, int W, const int32_t* corner_index, const float* desired, int P, const float* g, float* dx,
                       int accumulate, esr_stream_t stream);

/* ---- random-alternatives Z objective (csrc/esr_pairmin.hip; reference codes/Z_optimization.py:683-701) ----
 * x: fp32 [Bg][C][H][W], the GLOBAL batch, read as I = clamp(x, 0, 1) when clamp01 and as x otherwise (feature tensors); [lo, hi): the rows of
 * this call; mask: [H][W] or NULL; init: [init_batch][C][H][W] with init_batch 1 (broadcast) or hi - lo, or NULL (then w is ignored).  Per
 * element e = (c, h, w):  near(r, e) = min(1, min_{a != r} |I_r - I_a|),  v(r, e) = mask(h, w) (near(r, e) - w |I_r - init_r|).
 * An exact tie between neighbours goes to the LOWEST row index a, the diagonal (distance 1) counting as index r.
 * esr_pairmin: partial[r - lo][k] (doubles), k < esr_pairmin_blocks(C, H, W): workgroup k's part of sum_e v(r, e); the caller sums over k.
 *   No atomics: two calls give the same bits.
 * esr_pairmin_grad: dx [hi - lo][C][H][W] = scale * d/dx[lo:hi] of sum over ALL Bg rows r of sum_e v(r, e): a local row's own term and
 *   the terms it receives as the nearest neighbour of any row; nothing where the diagonal wins; sign(0) = 0; with clamp01 the gradient
 *   passes where 0 <= x <= 1.  Gather form, no atomics.
 * work: scratch of esr_pairmin_work_floats(...) floats (grad = 0 / 1 for the two calls), 0 (work may be NULL) whenever the Bg values of an
 *   element fit in LDS - Bg up to about 300; larger batches keep them in `work`.  Nothing of size Bg x Bg is allocated in either form. */
int64_t esr_pairmin_blocks(int C, int H, int W);
int64_t esr_pairmin_work_floats(int Bg, int C, int H, int W, int lo, int hi, int grad);
int esr_pairmin(const float* x, int Bg, int C, int H, int W, int lo, int hi, int clamp01, const float* mask, const float* init, int init_batch, float w,
                float* work, double* partial, esr_stream_t stream);
int esr_pairmin_grad(const float* x, int Bg, int C, int H, int W, int lo, int hi, int clamp01, const float* mask, const float* init, int init_batch,
                     float w, float scale, float* work, float* dx, esr_stream_t stream);

/* ---- the critic's glue: BatchNorm2d (training mode) + LeakyReLU, its gradient and the gradient of its gradient ----
 * Reference: Discriminator_VGG_128 (codes/models/modules/architecture.py:446-508): conv_block = nn.Conv2d -> nn.BatchNorm2d(affine, batch
 * statistics while training; block.py:25-35,129-146) -> LeakyReLU(0.2); the WGAN-GP penalty (codes/models/modules/loss.py:260-279)
 * differentiates the critic's input gradient, i.e. back-propagates through the BACKWARD of every one of these layers.  All three levels
 * are closed-form single-pass kernels on the conv kernels' activation layout (csrc/esr_critic.hip states the formulas):
 *   esr_bn_reduce mode 0 : sums[g][c] = (sum y, sum y^2)                                  esr_bn_finalize: mean, rstd, scale, shift, running stats
 *   esr_bn_apply  mode 0 : out0 = lrelu(scale*y + shift)                                  (torch: F.batch_norm(training=True) + leaky_relu)
 *   esr_bn_reduce mode 1 : sums[g][c] = (sum dyb, sum dyb*xhat),  dyb = dz * lrelu'       esr_bn_param_grads: dgamma, dbeta
 *   esr_bn_apply  mode 1 : out0 = d loss / d y                                            (autograd of the above)
 *   esr_bn_reduce mode 2 : sums[g][c] = (sum u, sum u*xhat, sum u*dyb)                    (u: cotangent of mode 1's result)
 *   esr_bn_apply  mode 2 : out0 = cotangent of dz, out1 = cotangent of y                  (torch: batchnorm_double_backward) + g_gamma via
 *                                                                                          esr_bn_param_grads
 * groups: the B images are `groups` runs of B/groups consecutive images, each normalised with its OWN batch statistics (the critic's
 * separate calls on the real, fake and interpolated batches executed as one launch); all per-channel arrays are [groups][C] except gamma /
 * beta / running_* ([C]).  scale == NULL: no normalisation (the first conv block has none) — then const_stats must be 1 (esr_bn_reduce and
 * esr_bn_apply return ESR_E_ARG otherwise).  const_stats: the affine map does not depend on y (eval-mode BatchNorm with running statistics,
 * or no norm).  s2d: dz (modes 1, 2), out0 of mode 0 and out0 of mode 2 are stored space-to-depth: logical pixel (y, x) of group cg at pixel
 * (y/2, x/2) of group 16*(cg/4) + 4*s + cg%4, s = 2*(y&1) + (x&1), of a view with H/2 x W/2 pixels (four consecutive groups share a parity) —
 * the input layout in which the next block's 4x4 stride-2 conv is a 3x3 stride-1 conv over 4x the channels.
 * View sizes: with n = ceil(C/8), y and every plain view must declare ncg >= n and H x W pixels; a space-to-depth view H/2 x W/2 pixels and
 * ncg >= 16*((n-1)/4) + (n-1)%4 + 13, one more than the largest group index above (4*n when n is a multiple of 4); ESR_E_ARG otherwise.
 * `sums` targets must be zeroed by the caller (the kernels add); sums2 / sums3: completed results of mode 1 / mode 2. */
typedef struct {
    esr_act_view y;          /* the conv's output (pre-normalisation); defines B x C x H x W */
    esr_act_view dz, u;      /* gradient w.r.t. the activated output (modes 1, 2); cotangent of mode 1's result (mode 2) */
    esr_act_view out0, out1;
    int32_t B, groups, C;
    const float* scale; const float* shift; const float* mean; const float* rstd;      /* [groups][C] */
    const float* gamma;      /* [C] or NULL (ones) */
    const double* sums2; const double* sums3;
    float slope;             /* LeakyReLU negative slope; 1.0f = no activation */
    int32_t const_stats, s2d;
} esr_bn_desc;
int esr_bn_reduce(const esr_bn_desc* d, int mode, double* sums, esr_stream_t stream);
int esr_bn_apply(const esr_bn_desc* d, int mode, esr_stream_t stream);
/* mean / rstd / scale (= gamma*rstd) / shift (= beta - scale*mean) from mode-0 sums, group by group IN ORDER; running_mean / running_var
 * (may be NULL) are updated once per group as nn.BatchNorm2d does per call: r = (1-momentum)*r + momentum*stat, variance unbiased. */
int esr_bn_finalize(const double* sums, int groups, int C, int64_t n_per_group, float eps, float momentum, const float* gamma, const float* beta,
                    float* mean, float* rstd, float* scale, float* shift, float* running_mean, float* running_var, esr_stream_t stream);
/* dgamma[c] = sum_g sums2[g][c][1], dbeta[c] = sum_g sums2[g][c][0]; g_gamma (double backward; needs sums3, rstd) — any output may be NULL */
int esr_bn_param_grads(const double* sums2, const double* sums3, const float* rstd, int groups, int C, int64_t n_per_group, float* dgamma, float* dbeta,
                       float* g_gamma, esr_stream_t stream);

/* ---- launch lists: a whole pass of the generator with ONE call ----
 * The reference dispatches every layer from Python (RRDBNet.forward's module loop, codes/models/modules/architecture.py:278-302, and
 * autograd's node-by-node backward); a port that keeps one FFI call per launch pays ~19 us of host time for each of the ~1,100 launches
 * of a training step.  The launch plan of a pass is static per (network, shape, precision, buffer set): the caller records it ONCE as an
 * array of esr_cmd — each entry is the argument block of one of the entry points above — and replays it with esr_run; between replays it
 * only patches the few pointers that change from call to call (the NCHW input / output tensors).  esr_run enqueues the commands in
 * order on `stream` and stops at the first one that fails: the return value is that command's ESR_E_* code and *failed (if given) its
 * index; ESR_OK and -1 otherwise.  Nothing is copied or retained: descriptors are read during the call only. */
enum {
    ESR_OP_CONV3X3 = 1, ESR_OP_PACK_NCHW = 2, ESR_OP_UNPACK_GRAD_NCHW = 3, ESR_OP_ACT_COMBINE = 4, ESR_OP_PIXEL_UNSHUFFLE = 5,
    ESR_OP_GRAD_ABSMAX = 6, ESR_OP_GRAD_SCALE = 7, ESR_OP_WGRAD_BATCH_RUN = 8, ESR_OP_PACK_BATCH_RUN = 9, ESR_OP_ZERO = 10,
    ESR_OP_UNPACK_NCHW = 11, ESR_OP_WGRAD = 12, ESR_OP_BN_REDUCE = 13, ESR_OP_BN_APPLY = 14, ESR_OP_BN_FINALIZE = 15, ESR_OP_BN_PARAM_GRADS = 16,
    ESR_OP_BN_FINALIZE_APPLY = 17
};
typedef struct { const float* src; int64_t src_batch_stride; int32_t B, C, h, w, c0, nc, pad, down; esr_act_view dst; } esr_cmd_pack_nchw;
typedef struct { esr_act_view G; float* dst; int64_t dst_batch_stride; int32_t B, C, h, w, c0, nc, pad, down, accumulate; } esr_cmd_unpack_grad_nchw;
/* A / Bv / mask with hi == NULL are absent (NULL in esr_act_combine) */
typedef struct { esr_act_view A; float alpha; esr_act_view Bv; float beta; int32_t s; esr_act_view mask; float mask_slope; esr_act_view out; int32_t B; } esr_cmd_act_combine;
typedef struct { esr_act_view src; int32_t r; esr_act_view dst; int32_t B; } esr_cmd_pixel_unshuffle;
typedef struct { esr_act_view v; int32_t B; uint32_t* slot; } esr_cmd_grad_absmax;
typedef struct { esr_act_view src, dst; int32_t B; const uint32_t* slot; int32_t exp; const float* scale_in; const float* scale_den; float* scale_out; } esr_cmd_grad_scale;
typedef struct { const void* workspace; esr_wgrad_batch_plan plan; } esr_cmd_wgrad_batch_run;
typedef struct { const void* workspace; int32_t n; int64_t nblocks; } esr_cmd_pack_batch_run;
typedef struct { void* p; int64_t n16; } esr_cmd_zero;
typedef struct { esr_act_view src; int32_t B, nc; float* dst; } esr_cmd_unpack_nchw;
typedef struct { esr_bn_desc d; int32_t mode; double* sums; } esr_cmd_bn;                 /* esr_bn_reduce (sums) / esr_bn_apply */
typedef struct { const double* sums; int32_t groups, C; int64_t n_per_group; float eps, momentum; const float* gamma; const float* beta;
                 float* mean; float* rstd; float* scale; float* shift; float* running_mean; float* running_var; } esr_cmd_bn_finalize;
typedef struct { const double* sums2; const double* sums3; const float* rstd; int32_t groups, C; int64_t n_per_group; float* dgamma; float* dbeta;
                 float* g_gamma; } esr_cmd_bn_param_grads;
/* esr_bn_finalize(f...) and esr_bn_apply(d, 0) as ONE launch: the normalise + activate kernel derives its affine from the mode-0 sums itself
 * (same fp64 arithmetic) and its first block per channel group stores mean / rstd / scale / shift and moves the running statistics.  d->scale,
 * d->shift, d->mean, d->rstd are not read (f's are written); f->groups, f->C, f->n_per_group must agree with d.  Nine launches fewer per
 * forward of Discriminator_VGG_128 (codes/models/modules/architecture.py:446-508). */
typedef struct { esr_bn_desc d; esr_cmd_bn_finalize f; } esr_cmd_bn_finalize_apply;
int esr_bn_finalize_apply(const esr_bn_desc* d, const esr_cmd_bn_finalize* f, esr_stream_t stream);
typedef struct {
    int32_t op;              /* ESR_OP_* */
    int32_t reserved;
    union {
        esr_conv3x3_desc conv;
        esr_cmd_pack_nchw pack_nchw;
        esr_cmd_unpack_grad_nchw unpack_grad_nchw;
        esr_cmd_act_combine act_combine;
        esr_cmd_pixel_unshuffle pixel_unshuffle;
        esr_cmd_grad_absmax grad_absmax;
        esr_cmd_grad_scale grad_scale;
        esr_cmd_wgrad_batch_run wgrad_batch_run;
        esr_cmd_pack_batch_run pack_batch_run;
        esr_cmd_zero zero;
        esr_cmd_unpack_nchw unpack_nchw;
        esr_wgrad_desc wgrad;
        esr_cmd_bn bn;
        esr_cmd_bn_finalize bn_finalize;
        esr_cmd_bn_param_grads bn_param_grads;
        esr_cmd_bn_finalize_apply bn_finalize_apply;
    } u;
} esr_cmd;
int esr_run(const esr_cmd* cmds, int n, int* failed, esr_stream_t stream);
/* `lanes` (1 .. ESR_MAX_LANES) INDEPENDENT launch lists side by side: lists that touch disjoint data (the sub-batches of an inference
 * forward), so that one list's launches fill the part-empty last tile round and the ramp of the other's.  cmds[l] / n[l] is lane l's list.
 * Lane 0 is enqueued on `main`, lanes 1.. on side streams the library owns (created once per device at first use, non-blocking, kept for
 * the life of the process; at most ESR_MAX_LANES - 1, so that with the caller's stream a process stays within HIP's default four hardware
 * queues).  The commands are issued interleaved — command i of every lane, then command i + 1 of every lane — not lane by lane.  The side
 * lanes start behind everything `main` held at the call (fork event) and `main` continues behind their last commands (join events): to the
 * caller the call is ordered on `main` like esr_run.  lanes == 1 is esr_run.  A failing command ends the issue with its ESR_E_* code,
 * *failed_lane / *failed (if given) its lane and index; the join is enqueued all the same.  ESR_E_ARG: lanes out of range, cmds or n NULL,
 * n[l] < 0, n[l] > 0 with cmds[l] NULL.  ESR_E_UNSUPPORTED: lanes > 1 while `main` is being captured into a graph.  Calls are serialised
 * inside the library (the side streams are shared by all callers of a device). */
#define ESR_MAX_LANES 4
int esr_run_lanes(const esr_cmd* const* cmds, const int* n, int lanes, int* failed_lane, int* failed, esr_stream_t main);
int64_t esr_cmd_bytes(void);       /* sizeof(esr_cmd): lets a binding check its struct layout */

/* ---- explorable JPEG decoding: the 8x8 block DCT consistency layer (codes/JPEG_module/JPEG.py, Y channel, block size 8) ----
 * Images are fp32 [B][1][H][W] (0...255), coefficients fp32 [B][64][h][w] with h = H/8, w = W/8 and channel 8u + v = vertical frequency u,
 * horizontal frequency v of the orthonormal DCT-II of the block at (i, j).  `qtab` is fp32 [B][64], row-major (u, v), one table per image
 * (JPEG.Set_Q_Table, JPEG.py:74-86).  The reference evaluates each transform by broadcasting against a [B,8,8,h,w,8] temporary per axis
 * (JPEG.py:108-120); here one launch per call moves each side once, in 16-byte accesses where the addresses allow (image and coefficient
 * pointers 16-byte aligned, w a multiple of 4; any w works).  Images must be 16-byte aligned.  No atomics: two calls give the same bits.
 * B and h up to 65535 (ESR_E_UNSUPPORTED beyond).
 *
 * esr_jpeg_compress — JPEG.forward with compress=True (JPEG.py:131-163): coef = DCT(x - 128) / qtab, torch.round (half to even) when
 *   round != 0.  H, W multiples of 8 (ESR_E_ARG otherwise).  act_out (optional; then coef may be NULL): the same values written into
 *   groups [0, 8) of the view in its format and planes (interior pixels only, as the conv kernels store), so that the generator's first conv
 *   reads them without a second pass (esr_pack_nchw). */
int esr_jpeg_compress(const float* x, int B, int H, int W, const float* qtab, int round, float* coef, const esr_act_view* act_out,
                      esr_stream_t stream);
/* esr_jpeg_extract — JPEG.forward with compress=False (JPEG.py:193-197) with the generator's tail in front of it
 *   (codes/models/modules/architecture.py:206, 214 after nn.Sigmoid): c = coef when y == NULL, else c = coef + (sigmoid(y) - 0.5) with y the
 *   last conv's fp32 [B][64][h][w] output and coef the quantised input; coef_out (optional) receives c;
 *   img[b][0][8i + r][8j + s] = 128 + iDCT(c * qtab). */
int esr_jpeg_extract(const float* coef, const float* y, int B, int h, int w, const float* qtab, float* coef_out, float* img,
                     esr_stream_t stream);
/* Adjoint of esr_jpeg_extract (autograd through JPEG.py:193-197 and the sigmoid): d_coef = qtab * DCT(d_img) — the transform is orthonormal,
 *   so the adjoint of the inverse is the forward transform — and, with y, d_y = d_coef * s (1 - s), s = sigmoid(y).  Either output may be NULL
 *   (not both); d_y needs y. */
int esr_jpeg_extract_grad(const float* d_img, const float* y, int B, int h, int w, const float* qtab, float* d_coef, float* d_y,
                          esr_stream_t stream);
/* Adjoint of the non-quantising compressor (autograd through JPEG.py:131-156): d_x = iDCT(d_coef / qtab).  (With rounding the reference's
 *   gradient is zero: no kernel.) */
int esr_jpeg_compress_grad(const float* d_coef, int B, int h, int w, const float* qtab, float* d_x, esr_stream_t stream);

/* ---- the colour model of the explorable JPEG decoder: the 16x16 block DCT of 4:2:0 chroma (codes/JPEG_module/JPEG.py, chroma_mode, block 16) ----
 * Images are fp32 [B][C][H][W] (YCbCr, 0...255), h = H/16, w = W/16.  Every image plane keeps K = 16 frequencies per axis (256 channels,
 * channel 16u + v) or K = 8 (64 channels, channel 8u + v, u, v < 8: dropping the rest is the chroma down-sampling; on the way back the missing
 * frequencies are zero).  `qtab` is fp32 [B][3][256]: per image the luminance table and twice the chrominance table, each edge-padded to 16x16
 * (JPEG.padded_Q_table), row-major (u, v); a K = 8 plane reads entries 16u + v.  Y is shifted by 128, Cb and Cr by 0.  One launch per call; one
 * workgroup owns 16 image rows x 16 blocks of one plane; 16-byte accesses on both sides where the addresses allow (pointers 16-byte aligned, w
 * a multiple of 4; any w works).  Images must be 16-byte aligned.  No atomics: two calls give the same bits.  B * planes and h up to 65535
 * (ESR_E_UNSUPPORTED beyond).
 *
 * esr_jpeg16_compress — JPEG.forward, compress=True, chroma_mode (JPEG.py:131-154) on a three-plane image; H, W multiples of 16.  mode:
 *   ESR_JPEG16_ALL         downsample_or_quantize=False: coef [B][768][h][w] = Y, Cb, Cr with K = 16 each, nothing rounded
 *   ESR_JPEG16_DOWNSAMPLE  'downsample_only': coef [B][384][h][w] = Y (K = 16) | Cb (K = 8) | Cr (K = 8), nothing rounded
 *   ESR_JPEG16_QUANTIZE    True: the same 384 channels with Cb and Cr rounded half to even (Y is never rounded, JPEG.py:144-148) */
#define ESR_JPEG16_ALL 0
#define ESR_JPEG16_DOWNSAMPLE 1
#define ESR_JPEG16_QUANTIZE 2
int esr_jpeg16_compress(const float* x, int B, int H, int W, const float* qtab, int mode, float* coef, esr_stream_t stream);
/* esr_jpeg16_extract — JPEG.forward, compress=False, chroma_mode (JPEG.py:165-201).  `form` is the reference's dispatch on the channel count:
 *   128 = Cb, Cr (K = 8) -> img [B][2][H][W];  512 = Cb, Cr (K = 16) -> [B][2][H][W];  384 = Y (K = 16) | Cb | Cr (K = 8) -> [B][3][H][W], +128 on Y.
 *   The `form` channels are read at channel coef_c0 of a tensor of coef_C channels (a slice of a wider tensor needs no copy).  With y (form 128
 *   only): the chroma generator's tail (architecture.py:206-212) in front, c = coef + (sigmoid(y) - 0.5) with y the last conv's fp32
 *   [B][128][h][w] output; coef_out (optional, with y) receives c as [B][128][h][w]. */
int esr_jpeg16_extract(const float* coef, int coef_C, int coef_c0, const float* y, int form, int B, int h, int w, const float* qtab,
                       float* coef_out, float* img, esr_stream_t stream);
/* Adjoint of esr_jpeg16_extract: d_coef [B][form][h][w] = qtab * DCT16(d_img) restricted to the kept frequencies and, with y (form 128),
 *   d_y = d_coef * s (1 - s), s = sigmoid(y).  Either output may be NULL (not both); d_y needs y. */
int esr_jpeg16_extract_grad(const float* d_img, const float* y, int form, int B, int h, int w, const float* qtab, float* d_coef, float* d_y,
                            esr_stream_t stream);
/* Adjoint of esr_jpeg16_compress: d_x [B][3][H][W] = iDCT16(d_coef / qtab) over the channels of `mode`.  ESR_JPEG16_QUANTIZE: only the Y plane
 *   is written (the rounded Cb and Cr planes have zero gradient, as torch.round's: the caller passes d_x zero-filled). */
int esr_jpeg16_compress_grad(const float* d_coef, int mode, int B, int h, int w, const float* qtab, float* d_x, esr_stream_t stream);

/* ---- the editing tools of the explorable JPEG decoder (codes/GUI.py imprinting; codes/models/DecompCNN_model.py:316-334) ----
 * esr_ycbcr_rgb — util.Tensor_YCbCR2RGB(x / 255) (codes/utils/util.py:328-330; the colour model's Output_Batch(within_0_1=True),
 *   DecompCNN_model.py:749-752) without its [B][3][3][H][W] broadcast: x fp32 [B][3][H][W] YCbCr in 0...255 -> rgb [B][3][H][W], un-clamped, in 0...1:
 *   rgb[r] = sum_c (float)(255 M[c][r]) (x[c] / 255) + (float)o[r] / 255 with the reference's M and o, in fp32.  One read and one write per value,
 *   16-byte accesses when H W is a multiple of 4 and both pointers are 16-byte aligned, element by element otherwise.  B up to 65535.
 * esr_ycbcr_rgb_grad — its adjoint: d_x[c] = (sum_r (float)(255 M[c][r]) d_rgb[r]) / 255. */
int esr_ycbcr_rgb(const float* x, int B, int H, int W, float* rgb, esr_stream_t stream);
int esr_ycbcr_rgb_grad(const float* d_rgb, int B, int H, int W, float* d_x, esr_stream_t stream);
/* esr_jpeg_violation — how far each of N candidate images leaves the set consistent with a compressed code (the imprint search,
 *   codes/GUI.py:1019-1033, which materialises the [N][64][h][w] coefficients of ~1300 candidates and retries in chunks when memory runs out):
 *   score[n] = sum over the 64 h w coefficients of max(0, |DCT(cand[n] - 128) / qtab - coef| - 0.5).  cand fp32 [N][1][H][W] (0...255, 16-byte
 *   aligned, H and W multiples of 8), coef fp32 [coef_n][64][h][w] and qtab fp32 [qtab_n][64] with coef_n, qtab_n = 1 (one for all) or N.  Terms in
 *   fp32, sums in fp64.  One workgroup owns 32 consecutive blocks (row-major over h w) of one candidate and writes one partial; `partial` is a
 *   workspace of N esr_jpeg_violation_partials(H, W) doubles, added per candidate in a fixed order by a second launch, no atomics: two calls give
 *   the same bits, and the coefficient tensor is never written.  Coefficients are read in 16-byte accesses when h w is a multiple of 4 and coef
 *   is 16-byte aligned, element by element otherwise, with the same bits.  N x partials up to 2^31 - 1.  No gradient. */
int64_t esr_jpeg_violation_partials(int H, int W);
int esr_jpeg_violation(const float* cand, int N, int H, int W, const float* coef, int coef_n, const float* qtab, int qtab_n, double* partial,
                       double* score, esr_stream_t stream);
/* esr_jpeg_pair — DecompCNN_model.py:320-324 in one launch: out = 128 + iDCT(qtab (clamp(DCT(desired - 128) / qtab - coef, -0.5, 0.5) + coef)), the
 *   image closest (per coefficient) to `desired` whose quantised code is coef.  desired, out fp32 [B][1][H][W] (16-byte aligned), coef fp32
 *   [B][64][h][w], qtab fp32 [B][64].  Tiling and access forms of esr_jpeg_violation.  No gradient. */
int esr_jpeg_pair(const float* desired, int B, int H, int W, const float* coef, const float* qtab, float* out, esr_stream_t stream);
/* esr_jpeg16_pair — DecompCNN_model.py:325-333 in one launch, for the two chroma planes (the last two of the desired_C = 2 or 3 planes of
 *   `desired`, fp32 [B][desired_C][H][W], H and W multiples of 16): all 256 frequencies of the 16x16 block DCT are divided by the padded table
 *   and multiplied back (the extractor's 512-channel form), and the low 8x8 (u, v < 8) are clamped to within 0.5 of the plane's 64 quantised
 *   coefficients in between, read at channel coef_c0 + 64 plane + 8u + v of a tensor of coef_C channels (the compressor's 384 channels with
 *   coef_c0 = 256, or its last 128 with 0).  qtab fp32 [B][3][256] as for esr_jpeg16_compress.  out fp32 [B][2][H][W].  Tile of
 *   esr_jpeg16_compress; coefficients in 16-byte accesses when w is a multiple of 4 and coef 16-byte aligned, with the same bits otherwise.
 *   No gradient. */
int esr_jpeg16_pair(const float* desired, int desired_C, int B, int H, int W, const float* coef, int coef_C, int coef_c0, const float* qtab,
                    float* out, esr_stream_t stream);

/* ---- JPEG files into the explorable decoder's inputs (no counterpart in the reference: its GUI.py:2425-2462 is marked as not working) ----
 * Host side: baseline entropy decoding, no device involved (csrc/esr_jpeg_parse.h).  Accepted: SOF0 / SOF1, 8-bit samples, ONE interleaved scan
 * of 1 component or of 3 components at 4:2:0 or 4:4:4, 8- and 16-bit DQT entries, tables redefined before the scan, APPn / COM, fill bytes,
 * 0xFF00 stuffing, DRI with RSTn.  ESR_E_UNSUPPORTED with info->reason ESR_JPEG_R_PROGRESSIVE (SOF2), _SOF_KIND (lossless, hierarchical),
 * _ARITHMETIC, _PRECISION (12-bit), _SCANS (non-interleaved or several scans), _SAMPLING (4:2:2, 4:4:0, ...), _COMPONENTS (2 or 4),
 * _COLORSPACE (three components that an Adobe APP14 segment with transform 0 marks as RGB: three components are read as YCbCr).
 * ESR_E_DATA with reason _TRUNCATED, _BAD_CODE (a code in no table, a category past 11 / 10), _RUN (a run past coefficient 63), _NO_TABLE,
 * _RST (a wrong restart number), _DIMENSION (zero width or height), _SEGMENT (a malformed segment), _NOT_JPEG (no SOI).  Bad input never
 * crashes and never spins: every read is checked against n and every loop is bounded by n or by the block count.  Both calls are
 * re-entrant (no state), so files may be decoded on several host threads at once.
 *
 * esr_jpeg_file_info   — reads up to the scan header.  mcus_h x mcus_w MCUs of blocks_per_mcu blocks (h[c] x v[c] of component c, in
 *   component order); blocks_h / blocks_w: the component's block grid, padded to whole MCUs; scan_blocks: blocks in the file;
 *   sof: 0 or 1; tq[c]: the component's table.  A one-component file reports h = v = 1 whatever it says (its scan is not interleaved).
 * esr_jpeg_file_decode — scan: scan_len >= 64 scan_blocks int16, filled in scan order (MCU after MCU, blocks in the MCU's order, 64 values per
 *   block in zigzag order, DC prediction undone); tables: 4 x 64 uint16 in natural order (row-major u, v; 0: never defined); info optional.
 *   ESR_E_ARG: a NULL pointer, n < 0, scan_len too small.  On failure scan may be partly written and tables are not. */
#define ESR_JPEG_R_PROGRESSIVE 1
#define ESR_JPEG_R_SOF_KIND 2
#define ESR_JPEG_R_ARITHMETIC 3
#define ESR_JPEG_R_PRECISION 4
#define ESR_JPEG_R_SCANS 5
#define ESR_JPEG_R_SAMPLING 6
#define ESR_JPEG_R_COMPONENTS 7
#define ESR_JPEG_R_COLORSPACE 8
#define ESR_JPEG_R_TRUNCATED 32
#define ESR_JPEG_R_BAD_CODE 33
#define ESR_JPEG_R_RUN 34
#define ESR_JPEG_R_NO_TABLE 35
#define ESR_JPEG_R_RST 36
#define ESR_JPEG_R_DIMENSION 37
#define ESR_JPEG_R_SEGMENT 38
#define ESR_JPEG_R_NOT_JPEG 39
typedef struct {
    int32_t width, height, components, sof, restart_interval, mcus_h, mcus_w, blocks_per_mcu, reason, reserved;
    int32_t h[4], v[4], tq[4], blocks_h[4], blocks_w[4];
    int64_t scan_blocks;
} esr_jpeg_info;
int esr_jpeg_file_info(const uint8_t* bytes, int64_t n, esr_jpeg_info* info);
int esr_jpeg_file_decode(const uint8_t* bytes, int64_t n, int16_t* scan, int64_t scan_len, uint16_t* tables, esr_jpeg_info* info);
/* esr_jpeg_file_unpack — device side: the scan-order buffer of ONE file (uploaded as it is, 16-byte aligned) into the models' tensors, one
 *   launch.  An MCU holds y_h x y_v Y blocks (1 x 1 or 2 x 2) and n_chroma (0 or 2) chroma blocks.
 *     y_out (optional) fp32 [64][mcus_h y_v][mcus_w y_h]: channel 8u + v of block (i, j) = the Y block's coefficient at zigzag position of
 *       (u, v), as float, + y_dc on channel 0 — JPEG.forward's coefficient layout on the 8 x 8 grid;
 *     c_out (optional, n_chroma = 2) fp32 [128][mcus_h][mcus_w]: Cb | Cr likewise, + c_dc on channels 0 and 64 — the colour model's chroma
 *       coefficients on its 16 x 16 grid for a 4:2:0 file;
 *     act_out (optional): y_out's values in groups [0, 8) of an activation view of image 0 (as esr_jpeg_compress's act_out).
 *   A workgroup stages 32 MCUs of one MCU row in LDS (16-byte reads of the scan buffer) and stores rows of consecutive blocks of one
 *   channel (consecutive addresses).  ESR_E_ARG, with nothing written: a NULL scan, no output, a non-positive count, y_h / y_v other than 1 x 1
 *   or 2 x 2, n_chroma other than 0 or 2, c_out without chroma blocks, scan not 16-byte aligned, an act_out of fewer than 8 groups, of another
 *   size or format.  ESR_E_UNSUPPORTED: more than 65535 MCU rows. */
int esr_jpeg_file_unpack(const int16_t* scan, int mcus_h, int mcus_w, int y_h, int y_v, int n_chroma, float y_dc, float c_dc, float* y_out,
                         float* c_out, const esr_act_view* act_out, esr_stream_t stream);

/* ---- scores of the SR output: PSNR, SSIM and the spread over Z samples (codes/utils/util.py:196-228, :340-391; codes/test.py:198-242) ----
 * esr_psnr_ssim — a and b are fp32 [B][C][H][W], C 1 or 3.  Every value becomes a pixel as util.tensor2img makes one, in fp32 and in this order:
 *   v = (clamp(x, lo, hi) - lo) / (hi - lo) (an IEEE division), p = 255 v, and with ESR_PIXELS_ROUND p = rint(p) (NumPy's .round(): half to
 *   even); ESR_PIXELS_RAW takes x as the pixel (an image that is in 0...255 already; lo and hi are not read).  `border` pixels are dropped on
 *   every side.  From p on the arithmetic is fp64, as util.calculate_psnr / util.ssim cast first:
 *     sums[b][0] = sum over the C H' W' pixels of (pa - pb)^2                                       (PSNR = 20 log10(255 / sqrt(sums[b][0] / (C H' W'))))
 *     sums[b][1] = sum over channels and over the (H' - 10)(W' - 10) windows that fit of the SSIM map (SSIM = sums[b][1] / (C (H' - 10)(W' - 10)))
 *   with the 11-tap Gaussian window of sigma 1.5 normalised to sum 1 (cv2.getGaussianKernel(11, 1.5), outer product), C1 = (0.01 255)^2,
 *   C2 = (0.03 255)^2.  Where H' or W' is below 11 no window fits and sums[b][1] = 0.  `partial` is a workspace of
 *   2 B esr_psnr_ssim_partials(C, H, W, border) doubles (one pair per workgroup); they are added in a fixed order, no atomics: two calls give the
 *   same bits.  B C and H' / 21 up to 65535 (ESR_E_UNSUPPORTED beyond). */
#define ESR_PIXELS_FLOAT 0
#define ESR_PIXELS_ROUND 1
#define ESR_PIXELS_RAW 2
int64_t esr_psnr_ssim_partials(int C, int H, int W, int border);
int esr_psnr_ssim(const float* a, const float* b, int B, int C, int H, int W, float lo, float hi, int quantize, int border, double* partial,
                  double* sums, esr_stream_t stream);
/* esr_sample_std — x is fp32 [S][B][C][H][W]: map[b][c][y][x] = 255 std_s clamp(x, 0, 1), the population STD (np.std, ddof 0) over the S samples
 *   (codes/test.py:224-233; the projection subtracted there is the same for every sample of an image and leaves the STD unchanged), two passes
 *   in fp64 per pixel, stored as fp32; sums[b] = the fp64 sum of the un-rounded values of image b.  S = 1 gives zeros.  `partial` is a workspace of
 *   B esr_sample_std_partials(C, H, W) doubles, added as above.  B up to 65535. */
int64_t esr_sample_std_partials(int C, int H, int W);
int esr_sample_std(const float* x, int S, int B, int C, int H, int W, float* map, double* partial, double* sums, esr_stream_t stream);

/* ---- scores and pictures of the JPEG decoder's output (codes/test_JPEG.py:165-327; utils/util.py:209-226 tensor2img's chroma branches) ----
 * The decoder's images are fp32 [B][C][H][W] in 0...255: C = 1 is a Y plane (chroma mode 'Y'), C = 3 is Y, Cb, Cr ('YCbCr').  One pixel
 * t = (Y, Cb, Cr) becomes the three 0...255 pixels p_j, j = 0 R, 1 G, 2 B, by this chain (util.tensor2img through data.util.ycbcr2rgb, :198-215),
 * in these formats and this order:
 *     a_c = t_c / 255f                                     fp32, IEEE division                          (img_np / 255)
 *     x_c = a_c * 255f                                     fp32                                         (ycbcr2rgb: img *= 255.)
 *     r_j = ((x_0 M[0][j] + x_1 M[1][j]) + x_2 M[2][j]) * 255.0 + off_j
 *                                                          fp64, every product and sum rounded on its own (no fused multiply-add), in this order
 *     q_j = (float)(r_j / 255.0)                           one rounding to fp32
 *     s_j = 255f * q_j                                     fp32
 *     p_j = rint(255f * ((clamp(s_j, lo, hi) - lo) / (hi - lo)))    fp32: esr_psnr_ssim's pixel with ESR_PIXELS_ROUND
 *   M = {{0.00456621, 0.00456621, 0.00456621}, {0, -0.00153632, 0.00791071}, {0.00625893, -0.00318811, 0}},
 *   off = {-222.921, 135.576, -276.836} (data.util.ycbcr2rgb's literals).  With C = 1 the chain starts at a_1 = a_2 = (float)(128.0 / 255.0), the
 *   reference's 128 / 255 * np.ones_like(img); its three outputs differ by up to 1e-3 before rounding, so all three are computed.
 *   (NumPy's own 3-term matmul may add in another order or fuse, one fp64 ulp away: that can move p_j only where the value before rint lies
 *   within about 1e-5 of a half-integer.)
 * esr_ycbcr_image — x -> out uint8 [B][H][W][3] in B, G, R order (what util.tensor2img returns and cv2.imwrite takes): p_2, p_1, p_0 of every
 *   pixel; one read per input value, 3 bytes out.  Where W is a multiple of 4, x is 16-byte and out 4-byte aligned, a thread owns four adjacent
 *   pixels and stores three whole dwords; otherwise one pixel, byte stores; the same bits either way.  B up to 65535.
 * esr_psnr_ssim_ycbcr — sums[b] as esr_psnr_ssim gives them, of the 3 x H' x W' pixels p_j of a[b] against those of the image that starts
 *   b_batch_stride * b elements into the second operand: b_batch_stride is C H W (b is [B][C][H][W]) or 0 (every image of a against the one image b).  The workgroup of
 *   channel j reads the C planes of both operands and keeps p_j; nothing converted is written.  `partial`: 2 B esr_psnr_ssim_ycbcr_partials(C, H,
 *   W, border) doubles.  3 B and H' / 21 up to 65535.  PSNR = 20 log10(255 / sqrt(sums[b][0] / (3 H' W'))), SSIM = sums[b][1] / (3 (H' - 10)(W' - 10)).
 * esr_sample_std_ycbcr — x is fp32 [S][B][C][H][W]: map[b][j][y][x] = the population STD over the S samples of p_j (np.std of the rounded uint8
 *   pixels, codes/test_JPEG.py:263; R, G, B planes), two passes in fp64 with the conversion repeated in the second, stored as fp32;
 *   sums[b] = the fp64 sum of the un-rounded values (mean = sums[b] / (3 H W)).  S = 1 gives zeros.  `partial`: B
 *   esr_sample_std_ycbcr_partials(C, H, W) doubles.  B up to 65535.
 * All: ESR_E_ARG, with nothing written, for a NULL pointer, C other than 1 or 3, B, S, H or W below 1, hi <= lo, a border that leaves nothing, a
 *   b_batch_stride other than the two above; ESR_E_UNSUPPORTED beyond the limits named. */
int esr_ycbcr_image(const float* x, int B, int C, int H, int W, float lo, float hi, uint8_t* out, esr_stream_t stream);
int64_t esr_psnr_ssim_ycbcr_partials(int C, int H, int W, int border);
int esr_psnr_ssim_ycbcr(const float* a, const float* b, int B, int C, int H, int W, int64_t b_batch_stride, float lo, float hi, int border,
                        double* partial, double* sums, esr_stream_t stream);
int64_t esr_sample_std_ycbcr_partials(int C, int H, int W);
int esr_sample_std_ycbcr(const float* x, int S, int B, int C, int H, int W, float lo, float hi, float* map, double* partial, double* sums,
                         esr_stream_t stream);

/* ---- LR/HR training batches from images resident on the device (codes/data/LRHR_dataset.py:48-131, codes/data/util.py:95-130) ----
 * One item of a batch: where its decoded image lies and which crop and augmentation were drawn for it.  Images are HWC uint8, 3 channels in BGR
 * order (cv2.imread's) or 1 channel.  H and W are the LOGICAL size: they may be smaller than what is stored (util.modcrop of the validation phase is
 * expressed this way) and every replicate-padding clamp uses them; `stride` is the stored row length in pixels.  (y0, x0) is the origin of the
 * ph x pw HR crop, both multiples of sf.  flags: util.augment's decisions, applied hflip, then vflip, then transpose.  lr != NULL: the LR image is
 * supplied (dataroot_LR), same channel count, lr_H x lr_W with row stride lr_stride, and is cropped at (y0 / sf, x0 / sf) instead of synthesised. */
#define ESR_DATA_HFLIP 1
#define ESR_DATA_VFLIP 2
#define ESR_DATA_TRANSPOSE 4       /* needs ph == pw */
typedef struct {
    const uint8_t* hr;
    const uint8_t* lr;
    int32_t H, W, stride, channels;
    int32_t y0, x0;
    int32_t flags;
    int32_t lr_H, lr_W, lr_stride;
} esr_data_item;
/* What a source pixel becomes (host struct, read during the call).
 *   ESR_DATA_MAP_RGB: every byte v becomes float(v) / 255 (an IEEE fp32 division: bit-identical to u8.astype(float32) / 255.); 3 channels are
 *     re-ordered BGR -> RGB; w, b, scale are not read.
 *   ESR_DATA_MAP_MIX: a 3-channel pixel becomes the ONE value ((w . (scale x)) / scale + b) / scale with x = float(bgr) / 255 and scale x in fp32,
 *     the rest in fp64, rounded to fp32 once — util.bgr2ycbcr(only_y=True) on a float32 image with w = (24.966, 128.553, 65.481), b = 16,
 *     scale = 255 (color 'y'); w = (0.114, 0.587, 0.299), b = 0, scale = 1 is a plain dot product (color 'gray').  1-channel sources pass through
 *     as v / 255.  The map is applied per source pixel, before the LR filter, as the reference converts img_HR before imresize. */
#define ESR_DATA_MAP_RGB 0
#define ESR_DATA_MAP_MIX 1
typedef struct { int32_t mode, reserved; double w[3]; double b; double scale; } esr_data_channel_map;
/* esr_data_lrhr_batch — hr fp32 [B][Co][ph][pw] and lr fp32 [B][Co][ph/sf][pw/sf] of B items in ONE launch; Co = 1 under ESR_DATA_MAP_MIX, else
 *   the items' channel count (the same for all).  Before augmentation, hr is the crop of the mapped image x and, with i0 = y0 / sf, j0 = x0 / sf,
 *   half = k / 2,
 *     lr[i][j] = sum_{u,v} taps[u][v] x[clamp(pre + sf (i0 + i) + half - u, 0, H - 1)][clamp(pre + sf (j0 + j) + half - v, 0, W - 1)]
 *   — CEM.imresize_CEM.imresize(x, [1 / sf]) of the WHOLE image (replicate padding at the IMAGE border, never at the crop's), cropped afterwards,
 *   for taps = rot90(upscale kernel / sf^2, 2), device fp32 [k][k], any 2-D kernel (k odd, <= 63), and pre = calc_strides' (in [0, sf)); fp32
 *   accumulation, u outer and v inner.  Items with an LR image get its plain crop through the same map; taps may be NULL when all have one.
 *   `items` is the HOST copy of the table (read during the call: the arguments are checked against it), `items_dev` the same B structs in device
 *   memory, which the kernel reads — the caller copies them on `stream` before the call (one pinned, asynchronous copy).
 *   ESR_E_ARG, with nothing written: a NULL pointer; sf < 1; ph or pw no multiple of sf; k even or > 63; pre outside [0, sf); an origin that
 *   is negative or no multiple of sf; a crop that leaves the logical image (or the LR image); channels other than 1 / 3 or differing Co;
 *   transpose with ph != pw; stride < W.  ESR_E_UNSUPPORTED: no tile fits on chip for (sf, k), or B > 65535.
 * esr_data_lrhr_plan — the launch plan, decided from (sf, k, pre) alone: tile_lo_win[0] = T, the LR tile side of a workgroup (T sf HR pixels),
 *   [1] = window pixels staged before the HR tile's first row / column, [2] = the window's side in source pixels.  T is the largest power of two
 *   up to 8 whose window fits 64 KiB of LDS at 4 bytes per pixel (at least two workgroups per CU): 8 for (sf 4, k 17) and for (sf 8, k 45), 4 for
 *   (sf 16, k 63).  Small tiles on purpose: a training batch is then some 1500 short workgroups, six or more resident per CU. */
int esr_data_lrhr_plan(int sf, int k, int pre, int32_t* tile_lo_win);
int esr_data_lrhr_batch(const esr_data_item* items, const esr_data_item* items_dev, int B, int sf, const float* taps, int k, int pre, int ph, int pw,
                        const esr_data_channel_map* map, float* hr, float* lr, esr_stream_t stream);

/* ---- Kernel estimation (KernelGAN) for E images in lock step (csrc/esr_kgan.hip; codes/KernelGAN/) ----
 * All tensors are dense fp32 with a leading estimation index E (and, for the critic, a pass index in front of it: the real and the fake forward of
 * one D step are the two passes of the same launches).  A launch is the only barrier; there are no atomics, every reduction has a fixed order:
 * two runs give the same bits, and estimation e of a batch gets the bits a batch of one gets.  Every entry point checks its arguments before it
 * touches the device: ESR_E_ARG for a NULL pointer, E outside 1..65535 or a non-positive size; ESR_E_UNSUPPORTED as said per function.
 *
 * The generator is linear (six bias-free convolutions), so it is applied as ONE 13 x 13 kernel k composed from its layers:
 * esr_kgan_compose — one layer of the composition: out[e][d] = sum_c in[e][c] (*) w[e][d][c], the full 2-D convolution of the s x s planes
 *   in [E][Cin][s][s] with the f x f filters w [E][Cout][Cin][f][f]; out [E][Cout][s+f-1][s+f-1].  The chain starts from in = the first layer's
 *   weights [E][C][7][7] and ends at k [E][1][13][13] = codes/KernelGAN/kernelGAN.py:58-63's curr_k.  ESR_E_UNSUPPORTED: Cin or Cout > 64, s+f-1 > 13.
 * esr_kgan_compose_bwd — its adjoint: din [E][Cin][s][s] and dw [E][Cout][Cin][f][f] from dout.
 * esr_kgan_apply — y [E][3][oh][ow] = (x corr k)[::2, ::2] per colour plane of the crop x [E][3][H][W], oh = (H - 13) / 2 + 1.  noise given:
 *   y_noisy = y + noise / 255.  bic_taps (device, 8 x 8) given: bic [E][oh][ow], the reference's bicubic term (stride 2, padding 3, shaved to y's
 *   size, every plane the SUM over the three input planes), and partial [E][esr_kgan_apply_blocks(H, W)] partial sums of (y - bic)^2.
 *   ESR_E_UNSUPPORTED: H or W odd or below 14 (a crop smaller than the shave).
 * esr_kgan_dk — dk [E][13][13] = d/dk of sum(dy * y) with dy = dgan (optional, [E][3][oh][ow]) + lam[e][0] * 2 / N * (y - bic) (when bic is given;
 *   N = 3 oh ow, so that is lambda_bicubic times the gradient of the mean squared distance).
 * esr_kgan_constraints — the terms on k: losses [E][5] = (bicubic = sum(partial) / n_outputs, sum2one, boundaries with `mask` [13][13], centralized,
 *   sparse) and dk += lam[e][1..4] times their gradients; lam [E][5] = (bicubic, sum2one, boundaries, centralized, sparse).  log given:
 *   log[e * log_stride + slot] = the bicubic loss (the learner's record).  (|k|^0.2 has no gradient at 0: it counts as 0 there.)
 * esr_kgan_gather — crops: out [E][3][S][S] = 2 (img + noise / 255) - 1 from resident CHW planes in [0, 1]; meta [E][3] = (offset in floats, H, W)
 *   and top_left [E][2], both in device memory; corners are clamped into the image.  ESR_E_UNSUPPORTED: S > 1024.
 *
 * The critic: conv 7x7 3->C, five [conv 1x1 C->C, BatchNorm, ReLU], conv 1x1 C->1, sigmoid; all convs spectrally normalised, with bias.
 * Its parameters are ONE flat vector per estimation, esr_kgan_d_param_count(C) floats: W0 [C][3][7][7], b0 [C]; for l = 1..5: W [C][C], b, gamma,
 * beta [C]; W6 [C], b6 [1].  The power-iteration vectors are one vector of esr_kgan_d_uv_count(C) floats: per layer u [Cout] then v [Cin kh kw].
 * ESR_E_UNSUPPORTED for all of them: C no multiple of 8 or outside 8..64; an input below 7 x 7 or with more than 2048 output positions.
 * npass is 1 or 2; per-pass tensors are [npass][E][...].
 * esr_kgan_d_spectral — one power iteration per pass and layer (pass 1 starts from pass 0's u), eps 1e-12: uv updated in place; per pass the
 *   normalised weights wn (the parameter layout, weight slots only), the u and v used (uv_used) and sigma [npass][E][7] = u^T W v.
 * esr_kgan_d_forward — x [npass][E][3][H][W] through the critic in training mode (batch statistics of the one image, biased variance, eps 1e-5).
 *   act and xhat [npass][E][6][C][P], rstd [npass][E][6][C] are kept for the backward (P = (H-6)(W-6)); pred [npass][E][P] is the sigmoid map,
 *   loss [npass][E] = mean |pred - label_pass|, dz6 [npass][E][P] = scale * d loss / d(pre-sigmoid).  gp given ([npass][E][param count]): the
 *   last layer's parameter gradients are written there.
 * esr_kgan_d_backward — from dz6 back to the input.  dz [npass][E][6][C][P] is work space.  gp given: the gradients of every parameter per pass,
 *   those of the weights taken at the NORMALISED weights.  dx given: [npass][E][3][H][W], the data gradient.  One of the two is required.
 * esr_kgan_d_finish — grad [E][param count] = sum over the passes, in pass order, of the gradient at the stored weights:
 *   (G - <G, Wn> u v^T) / sigma with u and v constants (torch.nn.utils.spectral_norm's backward), biases and BatchNorm parameters summed. */
int esr_kgan_compose(const float* in, const float* w, float* out, int E, int Cin, int Cout, int s, int f, esr_stream_t stream);
int esr_kgan_compose_bwd(const float* in, const float* w, const float* dout, float* din, float* dw, int E, int Cin, int Cout, int s, int f,
                         esr_stream_t stream);
int esr_kgan_apply_blocks(int H, int W);
int esr_kgan_apply(const float* x, const float* k, const float* bic_taps, const float* noise, float* y, float* y_noisy, float* bic, float* partial,
                   int E, int H, int W, esr_stream_t stream);
int esr_kgan_dk(const float* x, const float* y, const float* bic, const float* dgan, const float* lam, float* dk, int E, int H, int W,
                esr_stream_t stream);
int esr_kgan_constraints(const float* k, float* dk, const float* mask, const float* lam, const float* partial, int npartial, int n_outputs,
                         float* losses, float* log, int log_stride, int slot, int E, esr_stream_t stream);
int esr_kgan_gather(const float* imgs, const int64_t* meta, const int32_t* top_left, const float* noise, float* out, int E, int S,
                    esr_stream_t stream);
int esr_kgan_d_param_count(int C);
int esr_kgan_d_uv_count(int C);
int esr_kgan_d_spectral(const float* params, float* uv, float* wn, float* uv_used, float* sigma, int E, int C, int npass, esr_stream_t stream);
int esr_kgan_d_forward(const float* x, const float* params, const float* wn, float* act, float* xhat, float* rstd, float label0, float label1,
                       float scale, float* pred, float* loss, float* dz6, float* gp, int E, int C, int H, int W, int npass, esr_stream_t stream);
int esr_kgan_d_backward(const float* x, const float* params, const float* wn, const float* act, const float* xhat, const float* rstd,
                        const float* dz6, float* dz, float* gp, float* dx, int E, int C, int H, int W, int npass, esr_stream_t stream);
int esr_kgan_d_finish(const float* gp, const float* wn, const float* uv_used, const float* sigma, float* grad, int E, int C, int npass,
                      esr_stream_t stream);

int esr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ESR_HIP_H */
