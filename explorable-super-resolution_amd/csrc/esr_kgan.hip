// Kernel estimation (KernelGAN) for E images in lock step: small fp32 kernels, one launch per seam (include/esr_hip.h, "esr_kgan_*").
// Every kernel carries the estimation index in blockIdx.z and, for the critic, the pass (real / fake forward of one D step) in blockIdx.y.
// A launch is the only barrier: no workgroup waits on another, no atomics; every reduction is a fixed-order tree inside ONE workgroup
// (a workgroup owns a whole channel plane, a whole weight row or a whole 13 x 13 kernel), so two runs give the same bits and
// estimation e of a batch computes exactly what a batch of one computes.
#include "esr_common.h"

#define KG_T 256          // threads per workgroup, all kernels
#define KG_PP 8           // positions per thread a critic kernel keeps in registers: P <= KG_T * KG_PP
#define KG_KS 13          // side of the composed kernel
#define KG_KN 169
#define KG_DK 7           // side of the critic's first conv
#define KG_K0 147         // 3 * 7 * 7

// ---- the flat layouts of the critic's parameters and of its power-iteration vectors (mirrored by esr_hip/kernelgan.py)
// params: W0 [C][147], b0 [C], then for l = 1..5: W [C][C], b [C], gamma [C], beta [C], then W6 [C], b6 [1]
__host__ __device__ __forceinline__ int kg_base(int C, int l) { return l == 0 ? 0 : (KG_K0 + 1) * C + (l - 1) * (C * C + 3 * C); }
__host__ __device__ __forceinline__ int kg_cout(int C, int l) { return l == 6 ? 1 : C; }
__host__ __device__ __forceinline__ int kg_kdim(int C, int l) { return l == 0 ? KG_K0 : C; }
__host__ __device__ __forceinline__ int kg_off_b(int C, int l) { return kg_base(C, l) + kg_cout(C, l) * kg_kdim(C, l); }
__host__ __device__ __forceinline__ int kg_off_gamma(int C, int l) { return kg_off_b(C, l) + C; }
__host__ __device__ __forceinline__ int kg_off_beta(int C, int l) { return kg_off_b(C, l) + 2 * C; }
__host__ __device__ __forceinline__ int kg_nparams(int C) { return kg_base(C, 6) + C + 1; }
// uv: per layer u [Cout] then v [K]
__host__ __device__ __forceinline__ int kg_off_u(int C, int l) { return l == 0 ? 0 : C + KG_K0 + (l - 1) * 2 * C; }
__host__ __device__ __forceinline__ int kg_nuv(int C) { return kg_off_u(C, 6) + 1 + C; }

// sum over the workgroup, the same value in every thread; a fixed tree, so the result does not depend on timing
__device__ __forceinline__ float kg_block_sum(float v, float* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = KG_T / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double kg_block_sum_d(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = KG_T / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
// Long sums run as eight interleaved partial sums of short inner sums, combined as a tree: the chains stay short (rounding grows with the chain),
// and the order is fixed.
__device__ __forceinline__ float kg_tree8(const float (&a)[8]) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }
__device__ __forceinline__ float kg_wave_sum(float v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- G as one kernel: layer composition -----------------------------------------------------------------------------------------
// out[e][d] = sum_c in[e][c] (*) w[e][d][c], the FULL 2-D convolution: in is s x s, w is f x f, out is (s + f - 1) squared
__global__ __launch_bounds__(KG_T) void kg_compose_fwd(const float* __restrict__ in, const float* __restrict__ w, float* __restrict__ out,
                                                        int Cin, int Cout, int s, int f) {
    const int d = blockIdx.x, e = blockIdx.z, so = s + f - 1;
    in += (long long)e * Cin * s * s;
    w += ((long long)e * Cout + d) * Cin * f * f;
    out += ((long long)e * Cout + d) * so * so;
    for (int n = threadIdx.x; n < so * so; n += KG_T) {
        const int p = n / so, q = n % so;
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < Cin; c0 += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int c = c0 + u;
                if (c >= Cin) continue;
                float acc = 0.f;
                for (int i = 0; i < f; ++i) {
                    const int pi = p - i;
                    if (pi < 0 || pi >= s) continue;
                    for (int j = 0; j < f; ++j) {
                        const int qj = q - j;
                        if (qj < 0 || qj >= s) continue;
                        acc = fmaf(in[(c * s + pi) * s + qj], w[(c * f + i) * f + j], acc);
                    }
                }
                a[u] += acc;
            }
        }
        const float acc = kg_tree8(a);
        out[n] = acc;
    }
}

// the adjoint: workgroups [0, Cin) give din[e][c], workgroups [Cin, Cin + Cout) give dw[e][d]
__global__ __launch_bounds__(KG_T) void kg_compose_bwd(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ dout,
                                                        float* __restrict__ din, float* __restrict__ dw, int Cin, int Cout, int s, int f) {
    const int e = blockIdx.z, so = s + f - 1;
    in += (long long)e * Cin * s * s;
    w += (long long)e * Cout * Cin * f * f;
    dout += (long long)e * Cout * so * so;
    if ((int)blockIdx.x < Cin) {
        const int c = blockIdx.x;
        din += ((long long)e * Cin + c) * s * s;
        for (int n = threadIdx.x; n < s * s; n += KG_T) {
            const int p = n / s, q = n % s;
            float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int d0 = 0; d0 < Cout; d0 += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int d = d0 + u;
                    if (d >= Cout) continue;
                    float acc = 0.f;
                    for (int i = 0; i < f; ++i)
                        for (int j = 0; j < f; ++j)
                            acc = fmaf(dout[(d * so + p + i) * so + q + j], w[((d * Cin + c) * f + i) * f + j], acc);
                    a[u] += acc;
                }
            }
            din[n] = kg_tree8(a);
        }
    } else {
        const int d = blockIdx.x - Cin;
        dw += ((long long)e * Cout + d) * Cin * f * f;
        for (int n = threadIdx.x; n < Cin * f * f; n += KG_T) {
            const int c = n / (f * f), i = (n / f) % f, j = n % f;
            float acc = 0.f;
            for (int p = 0; p < s; ++p) {
                float row = 0.f;
                for (int q = 0; q < s; ++q) row = fmaf(in[(c * s + p) * s + q], dout[(d * so + p + i) * so + q + j], row);
                acc += row;
            }
            dw[n] = acc;
        }
    }
}

// ---- G as one kernel: y = (x corr k)[::2, ::2] per colour plane, the bicubic downscale of the same crop, and their squared distance ----
__global__ __launch_bounds__(KG_T) void kg_apply(const float* __restrict__ x, const float* __restrict__ k, const float* __restrict__ bict,
                                                  const float* __restrict__ noise, float* __restrict__ y, float* __restrict__ ynoisy,
                                                  float* __restrict__ bic, float* __restrict__ partial, int H, int W, int oh, int ow) {
    __shared__ float sk[KG_KN], sb[64], red[KG_T];
    const int e = blockIdx.z, t = threadIdx.x;
    if (t < KG_KN) sk[t] = k[e * KG_KN + t];
    if (bict && t < 64) sb[t] = bict[t];
    __syncthreads();
    x += (long long)e * 3 * H * W;
    const int n = blockIdx.x * KG_T + t, P = oh * ow;
    float sq = 0.f;
    if (n < P) {
        const int oy = n / ow, ox = n % ow;
        float yc[3];
        for (int c = 0; c < 3; ++c) {
            const float* xp = x + ((long long)c * H + 2 * oy) * W + 2 * ox;
            float acc = 0.f;
            for (int u = 0; u < KG_KS; ++u) {
                float row = 0.f;
                for (int v = 0; v < KG_KS; ++v) row = fmaf(xp[u * W + v], sk[u * KG_KS + v], row);
                acc += row;
            }
            yc[c] = acc;
            y[((long long)e * 3 + c) * P + n] = acc;
            if (ynoisy) ynoisy[((long long)e * 3 + c) * P + n] = acc + (noise ? noise[((long long)e * 3 + c) * P + n] / 255.f : 0.f);
        }
        if (bict) {
            // 8 x 8 taps, stride 2, padding 3, shaved by 3 outputs per side: rows 2 oy + 3 .. 2 oy + 10, always inside the crop
            float b = 0.f;
            for (int c = 0; c < 3; ++c) {
                const float* xp = x + ((long long)c * H + 2 * oy + 3) * W + 2 * ox + 3;
                for (int i = 0; i < 8; ++i) {
                    float row = 0.f;
                    for (int j = 0; j < 8; ++j) row = fmaf(xp[i * W + j], sb[i * 8 + j], row);
                    b += row;
                }
            }
            bic[(long long)e * P + n] = b;
            for (int c = 0; c < 3; ++c) sq = fmaf(yc[c] - b, yc[c] - b, sq);
        }
    }
    if (bict) {
        const float s = kg_block_sum(sq, red);
        if (t == 0) partial[e * gridDim.x + blockIdx.x] = s;
    }
}

// dk[e][u][v] = sum_{c, o} dy[e][c][o] x[e][c][2 oy + u][2 ox + v], dy = dgan (optional) + lam[e][0] * 2 / N * (y - bic)
__global__ __launch_bounds__(KG_T) void kg_dk(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ bic,
                                               const float* __restrict__ dgan, const float* __restrict__ lam, float* __restrict__ dk,
                                               int H, int W, int oh, int ow) {
    __shared__ float red[KG_T];
    const int e = blockIdx.z, u = blockIdx.x / KG_KS, v = blockIdx.x % KG_KS, P = oh * ow, N = 3 * P;
    x += (long long)e * 3 * H * W;
    const float coef = bic ? lam[e * 5] * 2.f / (float)N : 0.f;
    float acc = 0.f;
    for (int n = threadIdx.x; n < N; n += KG_T) {
        const int c = n / P, o = n % P, oy = o / ow, ox = o % ow;
        float g = dgan ? dgan[(long long)e * N + n] : 0.f;
        if (bic) g = fmaf(coef, y[(long long)e * N + n] - bic[(long long)e * P + o], g);
        acc = fmaf(g, x[((long long)c * H + 2 * oy + u) * W + 2 * ox + v], acc);
    }
    const float s = kg_block_sum(acc, red);
    if (threadIdx.x == 0) dk[e * KG_KN + blockIdx.x] = s;
}

// the five constraint terms on k and their gradient added to dk; losses[e] = (bicubic, sum2one, boundaries, centralized, sparse)
__global__ __launch_bounds__(KG_T) void kg_constraints(const float* __restrict__ k, float* __restrict__ dk, const float* __restrict__ mask,
                                                        const float* __restrict__ lam, const float* __restrict__ partial, int npartial, int N,
                                                        float* __restrict__ losses, float* __restrict__ log, int log_stride, int slot) {
    __shared__ float red[KG_T];
    const int e = blockIdx.z, t = threadIdx.x;
    const bool on = t < KG_KN;
    const float kv = on ? k[e * KG_KN + t] : 0.f, m = on ? mask[t] : 0.f;
    const float r = (float)(t / KG_KS), c = (float)(t % KG_KS);
    const float S = kg_block_sum(kv, red);
    const float R = kg_block_sum(kv * r, red), Cc = kg_block_sum(kv * c, red);
    const float bound = kg_block_sum(fabsf(kv * m), red) / (float)KG_KN;
    const float sparse = kg_block_sum(on ? powf(fabsf(kv), 0.2f) : 0.f, red) / (float)KG_KN;
    const float center = (float)(KG_KS / 2) + 0.5f * (2 - KG_KS % 2);
    const float cr = R / S, cc = Cc / S;
    const float cent = 0.5f * ((cr - center) * (cr - center) + (cc - center) * (cc - center));
    const float l1 = lam[e * 5 + 1], l2 = lam[e * 5 + 2], l3 = lam[e * 5 + 3], l4 = lam[e * 5 + 4];
    if (on) {
        float g = l1 * sgn(S - 1.f) + l2 * m * sgn(kv * m) / (float)KG_KN;
        if (l3 != 0.f) g += l3 * ((cr - center) * (r - cr) + (cc - center) * (c - cc)) / S;
        if (l4 != 0.f && kv != 0.f) g += l4 * 0.2f * powf(fabsf(kv), -0.8f) * sgn(kv) / (float)KG_KN;
        dk[e * KG_KN + t] += g;
    }
    if (t == 0) {
        float b = 0.f;
        for (int i = 0; i < npartial; ++i) b += partial[e * npartial + i];
        b /= (float)N;
        losses[e * 5 + 0] = b;
        losses[e * 5 + 1] = fabsf(1.f - S);
        losses[e * 5 + 2] = bound;
        losses[e * 5 + 3] = cent;
        losses[e * 5 + 4] = sparse;
        if (log) log[(long long)e * log_stride + slot] = b;
    }
}

// crops of side S from the resident images (CHW fp32 planes in [0, 1]) into [-1, 1]: out = 2 (img + noise / 255) - 1
__global__ __launch_bounds__(KG_T) void kg_gather(const float* __restrict__ imgs, const int64_t* __restrict__ meta, const int32_t* __restrict__ tl,
                                                   const float* __restrict__ noise, float* __restrict__ out, int S) {
    const int e = blockIdx.z, n = blockIdx.x * KG_T + threadIdx.x;
    if (n >= 3 * S * S) return;
    const int H = (int)meta[e * 3 + 1], W = (int)meta[e * 3 + 2];
    const int top = clampi(tl[e * 2], 0, H - S), left = clampi(tl[e * 2 + 1], 0, W - S);     // a bad table entry never reads outside the image
    const int c = n / (S * S), yy = (n / S) % S, xx = n % S;
    float v = imgs[meta[e * 3] + ((long long)c * H + top + yy) * W + left + xx];
    if (noise) v += noise[(long long)e * 3 * S * S + n] / 255.f;
    out[(long long)e * 3 * S * S + n] = v * 2.f - 1.f;
}

// ---- the critic ---------------------------------------------------------------------------------------------------------------------
// Spectral norm of the seven layers: workgroup (l, e) runs the power iteration of layer l once per pass (the second pass starts from the
// first's u), and leaves per pass the normalised weights W / sigma, the u and v it used and sigma.
__global__ __launch_bounds__(KG_T) void kg_spectral(const float* __restrict__ params, float* __restrict__ uv, float* __restrict__ wn,
                                                     float* __restrict__ uvs, float* __restrict__ sigma, int C, int npass) {
    __shared__ float su[64], sv[KG_K0], swv[64], red[KG_T];
    const int l = blockIdx.x, e = blockIdx.z, E = gridDim.z, t = threadIdx.x;
    const int co = kg_cout(C, l), K = kg_kdim(C, l), np = kg_nparams(C), nuv = kg_nuv(C);
    const float* Wm = params + (long long)e * np + kg_base(C, l);
    float* u = uv + (long long)e * nuv + kg_off_u(C, l);
    float* v = u + co;
    if (t < co) su[t] = u[t];
    __syncthreads();
    for (int pass = 0; pass < npass; ++pass) {
        // v = normalize(W^T u)
        float vj = 0.f;
        if (t < K)
            for (int i = 0; i < co; ++i) vj = fmaf(Wm[i * K + t], su[i], vj);
        float nrm = sqrtf(kg_block_sum(t < K ? vj * vj : 0.f, red));
        if (t < K) sv[t] = vj / fmaxf(nrm, 1e-12f);
        __syncthreads();
        // u = normalize(W v), a wave per row
        for (int i = t / 64; i < co; i += KG_T / 64) {
            float a = 0.f;
            for (int j = t % 64; j < K; j += 64) a = fmaf(Wm[i * K + j], sv[j], a);
            a = kg_wave_sum(a);
            if (t % 64 == 0) swv[i] = a;
        }
        __syncthreads();
        const float wv = t < co ? swv[t] : 0.f;
        nrm = sqrtf(kg_block_sum(wv * wv, red));
        const float un = wv / fmaxf(nrm, 1e-12f);
        const float sg = kg_block_sum(un * wv, red);
        if (t < co) su[t] = un;
        __syncthreads();
        float* wo = wn + ((long long)pass * E + e) * np + kg_base(C, l);
        for (int n = t; n < co * K; n += KG_T) wo[n] = Wm[n] / sg;
        float* us = uvs + ((long long)pass * E + e) * nuv + kg_off_u(C, l);
        if (t < co) us[t] = un;
        if (t < K) us[co + t] = sv[t];
        if (t == 0) sigma[((long long)pass * E + e) * 7 + l] = sg;
        __syncthreads();
    }
    if (t < co) u[t] = su[t];
    if (t < K) v[t] = sv[t];
}

// activations of one (pass, e): act[l] for l = 0..5 as [C][P]; xhat and dz share the shape
__device__ __forceinline__ long long kg_act_off(int pass, int E, int e, int l, int C, int P) { return ((((long long)pass * E + e) * 6 + l) * C) * P; }

// first layer: 7 x 7 conv 3 -> C with bias, no activation.  Workgroup (c, pass, e) owns one output plane.
__global__ __launch_bounds__(KG_T) void kg_d_first(const float* __restrict__ x, const float* __restrict__ wn, const float* __restrict__ params,
                                                    float* __restrict__ act, int C, int H, int W) {
    __shared__ float sw[KG_K0];
    const int c = blockIdx.x, pass = blockIdx.y, e = blockIdx.z, E = gridDim.z, t = threadIdx.x;
    const int oh = H - 6, ow = W - 6, P = oh * ow, np = kg_nparams(C);
    if (t < KG_K0) sw[t] = wn[((long long)pass * E + e) * np + c * KG_K0 + t];
    __syncthreads();
    const float b = params[(long long)e * np + kg_off_b(C, 0) + c];
    x += ((long long)pass * E + e) * 3 * H * W;
    float* out = act + kg_act_off(pass, E, e, 0, C, P) + (long long)c * P;
    for (int n = t; n < P; n += KG_T) {
        const int oy = n / ow, ox = n % ow;
        float acc = 0.f;
        for (int ci = 0; ci < 3; ++ci)
            for (int i = 0; i < KG_DK; ++i) {
                float row = 0.f;
                for (int j = 0; j < KG_DK; ++j) row = fmaf(x[((long long)ci * H + oy + i) * W + ox + j], sw[(ci * KG_DK + i) * KG_DK + j], row);
                acc += row;
            }
        out[n] = acc + b;
    }
}

// layer l = 1..5: 1 x 1 conv + bias, BatchNorm with the statistics of this plane (biased variance, eps), ReLU — one workgroup per plane
__global__ __launch_bounds__(KG_T) void kg_d_mid(const float* __restrict__ wn, const float* __restrict__ params, float* __restrict__ act,
                                                  float* __restrict__ xhat, float* __restrict__ rstd, int l, int C, int P, float eps) {
    __shared__ float sw[64], red[KG_T];
    const int c = blockIdx.x, pass = blockIdx.y, e = blockIdx.z, E = gridDim.z, t = threadIdx.x, np = kg_nparams(C);
    if (t < C) sw[t] = wn[((long long)pass * E + e) * np + kg_base(C, l) + c * C + t];
    __syncthreads();
    const float* pr = params + (long long)e * np;
    const float b = pr[kg_off_b(C, l) + c], gamma = pr[kg_off_gamma(C, l) + c], beta = pr[kg_off_beta(C, l) + c];
    const float* in = act + kg_act_off(pass, E, e, l - 1, C, P);
    float z[KG_PP], s = 0.f;
#pragma unroll
    for (int r = 0; r < KG_PP; ++r) {
        const int n = t + r * KG_T;
        z[r] = 0.f;
        if (n < P) {
            float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};        // C is a multiple of 8
            for (int c0 = 0; c0 < C; c0 += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] = fmaf(in[(long long)(c0 + u) * P + n], sw[c0 + u], a[u]);
            }
            const float acc = kg_tree8(a) + b;
            z[r] = acc;
            s += acc;
        }
    }
    const float mean = kg_block_sum(s, red) / (float)P;
    s = 0.f;
#pragma unroll
    for (int r = 0; r < KG_PP; ++r)
        if (t + r * KG_T < P) s = fmaf(z[r] - mean, z[r] - mean, s);
    const float rs = 1.f / sqrtf(kg_block_sum(s, red) / (float)P + eps);
    float* out = act + kg_act_off(pass, E, e, l, C, P) + (long long)c * P;
    float* xh = xhat + kg_act_off(pass, E, e, l, C, P) + (long long)c * P;
#pragma unroll
    for (int r = 0; r < KG_PP; ++r) {
        const int n = t + r * KG_T;
        if (n < P) {
            const float h = (z[r] - mean) * rs;
            xh[n] = h;
            out[n] = fmaxf(fmaf(gamma, h, beta), 0.f);
        }
    }
    if (t == 0) rstd[(((long long)pass * E + e) * 6 + l) * C + c] = rs;
}

// last layer: 1 x 1 conv C -> 1 + bias, sigmoid, L1 against the pass's label; the gradient at the pre-sigmoid map (times `scale`), and the
// layer's own parameter gradients when gp is given
__global__ __launch_bounds__(KG_T) void kg_d_last(const float* __restrict__ wn, const float* __restrict__ params, const float* __restrict__ act,
                                                   float label0, float label1, float scale, float* __restrict__ pred, float* __restrict__ loss,
                                                   float* __restrict__ dz6, float* __restrict__ gp, int C, int P) {
    // One workgroup per (pass, e) and a few thousand terms in all: the pre-sigmoid sum, the sigmoid and the two scalar sums (the loss, and the bias
    // gradient, whose terms cancel between positions) are taken in double, which costs nothing here and keeps these one-number results at one rounding.
    __shared__ float sw[64], sdz[KG_T * KG_PP];
    __shared__ double redd[KG_T];
    const int pass = blockIdx.y, e = blockIdx.z, E = gridDim.z, t = threadIdx.x, np = kg_nparams(C);
    const long long pe = (long long)pass * E + e;
    if (t < C) sw[t] = wn[pe * np + kg_base(C, 6) + t];
    __syncthreads();
    const float b = params[(long long)e * np + kg_off_b(C, 6)], label = pass ? label1 : label0;
    const float* in = act + kg_act_off(pass, E, e, 5, C, P);
    double l = 0., sd = 0.;
    for (int n = t; n < P; n += KG_T) {
        double acc = b;
        for (int ci = 0; ci < C; ++ci) acc += (double)in[(long long)ci * P + n] * (double)sw[ci];
        const double s = 1. / (1. + exp(-acc));
        l += fabs(s - (double)label);
        const double gd = (double)scale * (s > label ? 1. : (s < label ? -1. : 0.)) / (double)P * s * (1. - s);
        const float g = (float)gd;
        pred[pe * P + n] = (float)s;
        dz6[pe * P + n] = g;
        sdz[n] = g;
        sd += gd;
    }
    l = kg_block_sum_d(l, redd);
    sd = kg_block_sum_d(sd, redd);       // (also the barrier that makes sdz visible)
    if (t == 0) loss[pe] = (float)(l / (double)P);
    if (!gp) return;
    float* g = gp + pe * np;
    if (t == 0) g[kg_off_b(C, 6)] = (float)sd;
    for (int ci = t / 64; ci < C; ci += KG_T / 64) {
        float a = 0.f;
        for (int n = t % 64; n < P; n += 64) a = fmaf(sdz[n], in[(long long)ci * P + n], a);
        a = kg_wave_sum(a);
        if (t % 64 == 0) g[kg_base(C, 6) + ci] = a;
    }
}

// backward of layer l = 1..5 for channel c: the gradient at this plane's output from layer l + 1's dz, ReLU, BatchNorm, and (gp given) the
// gradients of gamma, beta, the bias and this row of the normalised weight
__global__ __launch_bounds__(KG_T) void kg_d_mid_bwd(const float* __restrict__ wn, const float* __restrict__ params, const float* __restrict__ act,
                                                      const float* __restrict__ xhat, const float* __restrict__ rstd, const float* __restrict__ dz6,
                                                      float* __restrict__ dz, float* __restrict__ gp, int l, int C, int P) {
    __shared__ float sw[64], red[KG_T], sdz[KG_T * KG_PP];
    const int c = blockIdx.x, pass = blockIdx.y, e = blockIdx.z, E = gridDim.z, t = threadIdx.x, np = kg_nparams(C);
    const long long pe = (long long)pass * E + e;
    const int Cn = kg_cout(C, l + 1);
    if (t < Cn) sw[t] = wn[pe * np + kg_base(C, l + 1) + t * C + c];
    __syncthreads();
    const float* dnext = l == 5 ? dz6 + pe * P : dz + kg_act_off(pass, E, e, l + 1, C, P);
    const float* a = act + kg_act_off(pass, E, e, l, C, P) + (long long)c * P;
    const float* xh = xhat + kg_act_off(pass, E, e, l, C, P) + (long long)c * P;
    float g[KG_PP], h[KG_PP], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int r = 0; r < KG_PP; ++r) {
        const int n = t + r * KG_T;
        g[r] = 0.f;
        h[r] = 0.f;
        if (n < P) {
            float pa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int c0 = 0; c0 < Cn; c0 += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (c0 + u < Cn) pa[u] = fmaf(dnext[(long long)(c0 + u) * P + n], sw[c0 + u], pa[u]);
            }
            const float acc = kg_tree8(pa);
            g[r] = a[n] > 0.f ? acc : 0.f;
            h[r] = xh[n];
            s1 += g[r];
            s2 = fmaf(g[r], h[r], s2);
        }
    }
    const float dbeta = kg_block_sum(s1, red), dgamma = kg_block_sum(s2, red);
    const float gamma = params[(long long)e * np + kg_off_gamma(C, l) + c], rs = rstd[(pe * 6 + l) * C + c];
    const float m1 = dbeta / (float)P, m2 = dgamma / (float)P;
    float* out = dz + kg_act_off(pass, E, e, l, C, P) + (long long)c * P;
    float sb = 0.f;
#pragma unroll
    for (int r = 0; r < KG_PP; ++r) {
        const int n = t + r * KG_T;
        if (n < P) {
            const float d = gamma * rs * (g[r] - m1 - h[r] * m2);
            out[n] = d;
            sdz[n] = d;
            sb += d;
        }
    }
    sb = kg_block_sum(sb, red);
    if (!gp) return;
    float* gq = gp + pe * np;
    if (t == 0) {
        gq[kg_off_b(C, l) + c] = sb;
        gq[kg_off_gamma(C, l) + c] = dgamma;
        gq[kg_off_beta(C, l) + c] = dbeta;
    }
    const float* in = act + kg_act_off(pass, E, e, l - 1, C, P);
    for (int ci = t / 64; ci < C; ci += KG_T / 64) {
        float acc = 0.f;
        for (int n = t % 64; n < P; n += 64) acc = fmaf(sdz[n], in[(long long)ci * P + n], acc);
        acc = kg_wave_sum(acc);
        if (t % 64 == 0) gq[kg_base(C, l) + c * C + ci] = acc;
    }
}

// backward of the first layer for channel c: dz0 from layer 1's dz, and (gp given) the bias and the 147 weight gradients
__global__ __launch_bounds__(KG_T) void kg_d_first_bwd(const float* __restrict__ x, const float* __restrict__ wn, float* __restrict__ dz,
                                                        float* __restrict__ gp, int C, int H, int W) {
    __shared__ float sw[64], red[KG_T], sdz[KG_T * KG_PP];
    const int c = blockIdx.x, pass = blockIdx.y, e = blockIdx.z, E = gridDim.z, t = threadIdx.x, np = kg_nparams(C);
    const int oh = H - 6, ow = W - 6, P = oh * ow;
    const long long pe = (long long)pass * E + e;
    if (t < C) sw[t] = wn[pe * np + kg_base(C, 1) + t * C + c];
    __syncthreads();
    const float* dnext = dz + kg_act_off(pass, E, e, 1, C, P);
    float* out = dz + kg_act_off(pass, E, e, 0, C, P) + (long long)c * P;
    float sb = 0.f;
    for (int n = t; n < P; n += KG_T) {
        float pa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};        // C is a multiple of 8
        for (int c0 = 0; c0 < C; c0 += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) pa[u] = fmaf(dnext[(long long)(c0 + u) * P + n], sw[c0 + u], pa[u]);
        }
        const float acc = kg_tree8(pa);
        out[n] = acc;
        sdz[n] = acc;
        sb += acc;
    }
    sb = kg_block_sum(sb, red);
    if (!gp) return;
    float* gq = gp + pe * np;
    if (t == 0) gq[kg_off_b(C, 0) + c] = sb;
    x += pe * 3 * H * W;
    for (int tap = t / 64; tap < KG_K0; tap += KG_T / 64) {
        const int ci = tap / 49, i = (tap / 7) % 7, j = tap % 7;
        float acc = 0.f;
        for (int n = t % 64; n < P; n += 64) acc = fmaf(sdz[n], x[((long long)ci * H + n / ow + i) * W + n % ow + j], acc);
        acc = kg_wave_sum(acc);
        if (t % 64 == 0) gq[c * KG_K0 + tap] = acc;
    }
}

// the gradient at the critic's input: dx[ci][y][x] = sum_c sum_ij Wn0[c][ci][i][j] dz0[c][y - i][x - j]
__global__ __launch_bounds__(KG_T) void kg_d_dx(const float* __restrict__ wn, const float* __restrict__ dz, float* __restrict__ dx, int C, int H, int W) {
    const int pass = blockIdx.y, e = blockIdx.z, E = gridDim.z, n = blockIdx.x * KG_T + threadIdx.x, np = kg_nparams(C);
    if (n >= 3 * H * W) return;
    const int oh = H - 6, ow = W - 6, P = oh * ow;
    const long long pe = (long long)pass * E + e;
    const int ci = n / (H * W), yy = (n / W) % H, xx = n % W;
    const float* w0 = wn + pe * np;
    const float* d0 = dz + kg_act_off(pass, E, e, 0, C, P);
    float pa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};        // C is a multiple of 8
    for (int c0 = 0; c0 < C; c0 += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = c0 + u;
            float acc = 0.f;
            for (int i = 0; i < KG_DK; ++i) {
                const int py = yy - i;
                if (py < 0 || py >= oh) continue;
                for (int j = 0; j < KG_DK; ++j) {
                    const int px = xx - j;
                    if (px < 0 || px >= ow) continue;
                    acc = fmaf(w0[c * KG_K0 + (ci * KG_DK + i) * KG_DK + j], d0[(long long)c * P + py * ow + px], acc);
                }
            }
            pa[u] += acc;
        }
    }
    dx[pe * 3 * H * W + n] = kg_tree8(pa);
}

// from the per-pass gradients at the normalised weights to the gradient at the stored ones, summed over the passes in pass order:
// dW_orig = (G - <G, Wn> u v^T) / sigma with u, v constants; the other parameters are plain sums
__global__ __launch_bounds__(KG_T) void kg_d_finish(const float* __restrict__ gp, const float* __restrict__ wn, const float* __restrict__ uvs,
                                                     const float* __restrict__ sigma, float* __restrict__ grad, int C, int npass) {
    __shared__ float red[KG_T];
    const int l = blockIdx.x, e = blockIdx.z, E = gridDim.z, t = threadIdx.x;
    const int co = kg_cout(C, l), K = kg_kdim(C, l), np = kg_nparams(C), nuv = kg_nuv(C), base = kg_base(C, l);
    float* go = grad + (long long)e * np;
    for (int pass = 0; pass < npass; ++pass) {
        const long long pe = (long long)pass * E + e;
        const float* G = gp + pe * np + base;
        const float* Wm = wn + pe * np + base;
        const float* u = uvs + pe * nuv + kg_off_u(C, l);
        const float* v = u + co;
        const float sg = sigma[pe * 7 + l];
        float d = 0.f;
        for (int n = t; n < co * K; n += KG_T) d = fmaf(G[n], Wm[n], d);
        d = kg_block_sum(d, red);
        for (int n = t; n < co * K; n += KG_T) {
            const float g = (G[n] - d * u[n / K] * v[n % K]) / sg;
            go[base + n] = pass ? go[base + n] + g : g;
        }
        const int nrest = l == 0 || l == 6 ? co : 3 * C;      // bias (, gamma, beta) follow the weight
        for (int n = t; n < nrest; n += KG_T) {
            const float g = gp[pe * np + base + co * K + n];
            go[base + co * K + n] = pass ? go[base + co * K + n] + g : g;
        }
    }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------
static bool kg_bad_E(int E) { return E < 1 || E > 65535; }
static int kg_check_C(int C) { return C < 8 || C > 64 || C % 8 ? ESR_E_UNSUPPORTED : ESR_OK; }

extern "C" {

int esr_kgan_d_param_count(int C) { return kg_check_C(C) ? kg_check_C(C) : kg_nparams(C); }
int esr_kgan_d_uv_count(int C) { return kg_check_C(C) ? kg_check_C(C) : kg_nuv(C); }

int esr_kgan_compose(const float* in, const float* w, float* out, int E, int Cin, int Cout, int s, int f, esr_stream_t stream) {
    if (!in || !w || !out || kg_bad_E(E) || Cin < 1 || Cout < 1 || s < 1 || f < 1) return ESR_E_ARG;
    if (Cin > 64 || Cout > 64 || s + f - 1 > KG_KS) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    kg_compose_fwd<<<dim3(Cout, 1, E), KG_T, 0, (hipStream_t)stream>>>(in, w, out, Cin, Cout, s, f);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

int esr_kgan_compose_bwd(const float* in, const float* w, const float* dout, float* din, float* dw, int E, int Cin, int Cout, int s, int f,
                         esr_stream_t stream) {
    if (!in || !w || !dout || !din || !dw || kg_bad_E(E) || Cin < 1 || Cout < 1 || s < 1 || f < 1) return ESR_E_ARG;
    if (Cin > 64 || Cout > 64 || s + f - 1 > KG_KS) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    kg_compose_bwd<<<dim3(Cin + Cout, 1, E), KG_T, 0, (hipStream_t)stream>>>(in, w, dout, din, dw, Cin, Cout, s, f);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

static int kg_check_crop(int H, int W) {
    if (H < 1 || W < 1) return ESR_E_ARG;
    if (H % 2 || W % 2 || H < KG_KS + 1 || W < KG_KS + 1) return ESR_E_UNSUPPORTED;     // smaller than the shave, or odd (the bicubic shave assumes even)
    return ESR_OK;
}

int esr_kgan_apply_blocks(int H, int W) {
    if (kg_check_crop(H, W)) return kg_check_crop(H, W);
    return (((H - KG_KS) / 2 + 1) * ((W - KG_KS) / 2 + 1) + KG_T - 1) / KG_T;
}

int esr_kgan_apply(const float* x, const float* k, const float* bic_taps, const float* noise, float* y, float* y_noisy, float* bic, float* partial,
                   int E, int H, int W, esr_stream_t stream) {
    if (!x || !k || !y || kg_bad_E(E) || (bic_taps && (!bic || !partial)) || (noise && !y_noisy)) return ESR_E_ARG;
    if (kg_check_crop(H, W)) return kg_check_crop(H, W);
    const int oh = (H - KG_KS) / 2 + 1, ow = (W - KG_KS) / 2 + 1;
    ESR_CLEAR_ERR();
    kg_apply<<<dim3((oh * ow + KG_T - 1) / KG_T, 1, E), KG_T, 0, (hipStream_t)stream>>>(x, k, bic_taps, noise, y, y_noisy, bic, partial, H, W, oh, ow);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

int esr_kgan_dk(const float* x, const float* y, const float* bic, const float* dgan, const float* lam, float* dk, int E, int H, int W,
                esr_stream_t stream) {
    if (!x || !dk || kg_bad_E(E) || (bic && (!y || !lam)) || (!bic && !dgan)) return ESR_E_ARG;
    if (kg_check_crop(H, W)) return kg_check_crop(H, W);
    const int oh = (H - KG_KS) / 2 + 1, ow = (W - KG_KS) / 2 + 1;
    ESR_CLEAR_ERR();
    kg_dk<<<dim3(KG_KN, 1, E), KG_T, 0, (hipStream_t)stream>>>(x, y, bic, dgan, lam, dk, H, W, oh, ow);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

int esr_kgan_constraints(const float* k, float* dk, const float* mask, const float* lam, const float* partial, int npartial, int n_outputs,
                         float* losses, float* log, int log_stride, int slot, int E, esr_stream_t stream) {
    if (!k || !dk || !mask || !lam || !partial || !losses || kg_bad_E(E) || npartial < 1 || n_outputs < 1) return ESR_E_ARG;
    if (log && (slot < 0 || slot >= log_stride)) return ESR_E_ARG;
    ESR_CLEAR_ERR();
    kg_constraints<<<dim3(1, 1, E), KG_T, 0, (hipStream_t)stream>>>(k, dk, mask, lam, partial, npartial, n_outputs, losses, log, log_stride, slot);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

int esr_kgan_gather(const float* imgs, const int64_t* meta, const int32_t* top_left, const float* noise, float* out, int E, int S,
                    esr_stream_t stream) {
    if (!imgs || !meta || !top_left || !out || kg_bad_E(E) || S < 1) return ESR_E_ARG;
    if (S > 1024) return ESR_E_UNSUPPORTED;
    ESR_CLEAR_ERR();
    kg_gather<<<dim3((3 * S * S + KG_T - 1) / KG_T, 1, E), KG_T, 0, (hipStream_t)stream>>>(imgs, meta, top_left, noise, out, S);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

static int kg_check_d(int E, int C, int H, int W, int npass) {
    if (kg_bad_E(E) || npass < 1 || npass > 2 || H < 1 || W < 1) return ESR_E_ARG;
    if (kg_check_C(C)) return kg_check_C(C);
    if (H < KG_DK || W < KG_DK || (H - 6) * (W - 6) > KG_T * KG_PP) return ESR_E_UNSUPPORTED;
    return ESR_OK;
}

int esr_kgan_d_spectral(const float* params, float* uv, float* wn, float* uv_used, float* sigma, int E, int C, int npass, esr_stream_t stream) {
    if (!params || !uv || !wn || !uv_used || !sigma) return ESR_E_ARG;
    if (kg_check_d(E, C, KG_DK, KG_DK, npass)) return kg_check_d(E, C, KG_DK, KG_DK, npass);
    ESR_CLEAR_ERR();
    kg_spectral<<<dim3(7, 1, E), KG_T, 0, (hipStream_t)stream>>>(params, uv, wn, uv_used, sigma, C, npass);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

int esr_kgan_d_forward(const float* x, const float* params, const float* wn, float* act, float* xhat, float* rstd, float label0, float label1,
                       float scale, float* pred, float* loss, float* dz6, float* gp, int E, int C, int H, int W, int npass, esr_stream_t stream) {
    if (!x || !params || !wn || !act || !xhat || !rstd || !pred || !loss || !dz6) return ESR_E_ARG;
    if (kg_check_d(E, C, H, W, npass)) return kg_check_d(E, C, H, W, npass);
    const int P = (H - 6) * (W - 6);
    hipStream_t st = (hipStream_t)stream;
    ESR_CLEAR_ERR();
    kg_d_first<<<dim3(C, npass, E), KG_T, 0, st>>>(x, wn, params, act, C, H, W);
    for (int l = 1; l <= 5; ++l) kg_d_mid<<<dim3(C, npass, E), KG_T, 0, st>>>(wn, params, act, xhat, rstd, l, C, P, 1e-5f);
    kg_d_last<<<dim3(1, npass, E), KG_T, 0, st>>>(wn, params, act, label0, label1, scale, pred, loss, dz6, gp, C, P);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

int esr_kgan_d_backward(const float* x, const float* params, const float* wn, const float* act, const float* xhat, const float* rstd,
                        const float* dz6, float* dz, float* gp, float* dx, int E, int C, int H, int W, int npass, esr_stream_t stream) {
    if (!x || !params || !wn || !act || !xhat || !rstd || !dz6 || !dz || (!gp && !dx)) return ESR_E_ARG;
    if (kg_check_d(E, C, H, W, npass)) return kg_check_d(E, C, H, W, npass);
    const int P = (H - 6) * (W - 6);
    hipStream_t st = (hipStream_t)stream;
    ESR_CLEAR_ERR();
    for (int l = 5; l >= 1; --l) kg_d_mid_bwd<<<dim3(C, npass, E), KG_T, 0, st>>>(wn, params, act, xhat, rstd, dz6, dz, gp, l, C, P);
    kg_d_first_bwd<<<dim3(C, npass, E), KG_T, 0, st>>>(x, wn, dz, gp, C, H, W);
    if (dx) kg_d_dx<<<dim3((3 * H * W + KG_T - 1) / KG_T, npass, E), KG_T, 0, st>>>(wn, dz, dx, C, H, W);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

int esr_kgan_d_finish(const float* gp, const float* wn, const float* uv_used, const float* sigma, float* grad, int E, int C, int npass,
                      esr_stream_t stream) {
    if (!gp || !wn || !uv_used || !sigma || !grad) return ESR_E_ARG;
    if (kg_check_d(E, C, KG_DK, KG_DK, npass)) return kg_check_d(E, C, KG_DK, KG_DK, npass);
    ESR_CLEAR_ERR();
    kg_d_finish<<<dim3(7, 1, E), KG_T, 0, (hipStream_t)stream>>>(gp, wn, uv_used, sigma, grad, C, npass);
    ESR_CHECK_LAUNCH();
    return ESR_OK;
}

}  // extern "C"
