// hav_stage2.hip -- kernels only stage-two (HD) training needs, gfx950.
//
// hav_haar_down2: the wavelet-domain down-sampling of FromRGB(use_wt=True) (model/styleUnet.py:453-458 of the reference:
// input = dwt(downsample(iwt(input))): InverseHaarTransform -> Downsample (4x4 FIR, down 2, pad (1, 1)) -> HaarTransform) as ONE pass,
// [B,4C,H,W] -> [B,4C,H/2,W/2], times `scale`.  It is the twin of hav_haar_up2 (hav_ops.hip) and keeps its conventions: channel = band*C + c,
// the three kernel banks exactly as the upfirdn2d calls receive them (unflipped).  With scale = 4 and the banks flipped it is the adjoint of
// hav_haar_up2, which is how the autograd nodes of native/train_ops.py use it.
//
// A thread produces 4 output columns of one (plane, output row) in all four bands.  An output coefficient reads a 4 x 4 neighbourhood of
// input positions in every band; the thread's footprint is 4 input rows x 10 input columns x 4 bands: per row and band two 16-byte loads
// of its own 8 columns (disjoint between lanes) and one 4-byte halo load on either side, which the neighbouring lane's lines already
// brought into the L1.  The rows are consumed in ascending order:
//   input row r  ->  the one or two synthesised rows it carries (hav_haar_idwt's arithmetic: one rounded product per band, summed
//                    ((ll + lh) + hl) + hh), 18 columns each
//                ->  FMA into the 2 x 8 decimated pixels they are taps of (the decimating kernels' chain: tap row i ascending, then j,
//                    flipped FIR, zeros outside the image)
// and the four band values of each output come from their 2 x 2 block of decimated pixels (hav_haar_dwt's FMA chain).  Every stage repeats
// the unfused kernel's operations in its order, so at scale 1 the result equals hav_haar_idwt -> hav_upfirdn2d -> hav_haar_dwt bit for bit,
// and at a power-of-two scale exactly that multiple (one more rounded product, exact short of overflow / underflow).
// Edges: addresses are clamped into the plane and the loaded value is replaced by zero (a synthesised pixel of zero inputs is a zero tap).
// One item per thread, no grid cap and no loop; no LDS, no atomics, no allocation, no synchronisation: the launch can be captured.
#include "hav_common.h"

// individually rounded product / sum, opaque to FMA contraction (as in hav_ops.hip)
__device__ __forceinline__ float s2_mul(float a, float b) { float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float s2_add(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// VEC: W % 8 == 0 and both tensors 16-byte aligned -- every thread's 8 own columns exist and load as two float4, its 4 outputs store as one.
template <bool VEC>
__global__ void __launch_bounds__(256) haar_down2_kernel(float* __restrict__ out, const float* __restrict__ in, const float* __restrict__ ki,
                                                         const float* __restrict__ fir, const float* __restrict__ kd, float scale,
                                                         int B, int C, int H, int W, int64_t total)
{
    const int OH = H >> 1, OW = W >> 1, OW4 = (OW + 3) >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float ks[16], kf[16], ka[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { ks[q] = ki[q]; ka[q] = kd[q]; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) kf[i * 4 + j] = fir[(3 - i) * 4 + (3 - j)];          // flipped FIR (upfirdn2d_kernel.cu:136-137)
    const int x4 = (int)(idx % OW4);
    const int64_t t = idx / OW4;
    const int oy = (int)(t % OH);
    const int64_t n = t / OH;          // plane b*C + c
    const int64_t b = n / C, c = n - b * C;
    const int c0 = 8 * x4;             // first own input column; the footprint is columns c0 - 1 .. c0 + 8

    // decimated pixels D[2 oy + q][c0 + p], q = 0..1, p = 0..7
    float acc[2][8];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int p = 0; p < 8; ++p) acc[q][p] = 0.f;

#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int iy = 2 * oy - 1 + r;
        const bool rok = iy >= 0 && iy < H;
        const int iyc = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
        float v[4][10];
#pragma unroll
        for (int band = 0; band < 4; ++band) {
            const float* row = in + ((((b * 4 + band) * C + c) * (int64_t)H + iyc) * (int64_t)W);
            const int xl = c0 - 1, xr = c0 + 8;
            const float hl = row[xl < 0 ? 0 : xl], hr = row[xr >= W ? W - 1 : xr];
            v[band][0] = (rok && xl >= 0) ? hl : 0.f;
            v[band][9] = (rok && xr < W) ? hr : 0.f;
            if constexpr (VEC) {
                const float4 a0 = *reinterpret_cast<const float4*>(row + c0), a1 = *reinterpret_cast<const float4*>(row + c0 + 4);
                v[band][1] = rok ? a0.x : 0.f; v[band][2] = rok ? a0.y : 0.f; v[band][3] = rok ? a0.z : 0.f; v[band][4] = rok ? a0.w : 0.f;
                v[band][5] = rok ? a1.x : 0.f; v[band][6] = rok ? a1.y : 0.f; v[band][7] = rok ? a1.z : 0.f; v[band][8] = rok ? a1.w : 0.f;
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int x = c0 + q;
                    const float e = row[x >= W ? W - 1 : x];
                    v[band][1 + q] = (rok && x < W) ? e : 0.f;
                }
            }
        }
        // the synthesised rows this input row carries: image row 4 oy - 1 + a, a = 2 r - 1 + ry (a = 0..5 are the six rows the two
        // decimated rows are taps of); columns 16 x4 - 1 + e, e = 0..17: input column index (e + 1) >> 1 of v, parity (e + 1) & 1
#pragma unroll
        for (int ry = 0; ry < 2; ++ry) {
            const int a = 2 * r - 1 + ry;
            if (a < 0 || a > 5) continue;
            float I[18];
#pragma unroll
            for (int e = 0; e < 18; ++e) {
                const int q = (e + 1) >> 1, kq = 2 * ry + ((e + 1) & 1);
                float s = s2_mul(v[0][q], ks[kq]);
                s = s2_add(s, s2_mul(v[1][q], ks[4 + kq]));
                s = s2_add(s, s2_mul(v[2][q], ks[8 + kq]));
                s = s2_add(s, s2_mul(v[3][q], ks[12 + kq]));
                I[e] = s;
            }
            // decimated row q sees synthesised row a as its tap row i = a - 2 q; tap column j of pixel p is column e = 2 p + j
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = a - 2 * q;
                if (i < 0 || i > 3) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int p = 0; p < 8; ++p) acc[q][p] = fmaf(I[2 * p + j], kf[i * 4 + j], acc[q][p]);
            }
        }
    }
    // analysis: band value of output (oy, 4 x4 + tq) from D[0..1][2 tq .. 2 tq + 1], taps (i, j) with the flipped 2x2 kernel
#pragma unroll
    for (int band = 0; band < 4; ++band) {
        const float* kb = ka + 4 * band;
        float o[4];
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) {
            float w = fmaf(acc[0][2 * tq], kb[3], 0.f);
            w = fmaf(acc[0][2 * tq + 1], kb[2], w);
            w = fmaf(acc[1][2 * tq], kb[1], w);
            w = fmaf(acc[1][2 * tq + 1], kb[0], w);
            o[tq] = s2_mul(w, scale);
        }
        float* dst = out + ((((b * 4 + band) * C + c) * OH + oy) * (int64_t)OW) + 4 * x4;
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int tq = 0; tq < 4; ++tq)
                if (4 * x4 + tq < OW) dst[tq] = o[tq];
        }
    }
}

extern "C" int hav_haar_down2(float* out, const float* in, const float* ki4x2x2, const float* fir4x4, const float* kd4x2x2, float scale,
                              int B, int C, int H, int W, void* stream)
{
    if (!out || !in || !ki4x2x2 || !fir4x4 || !kd4x2x2 || B < 1 || C < 1 || H < 1 || W < 1) return HAV_EINVAL;
    if ((H & 1) || (W & 1)) return HAV_EUNSUP;
    const int64_t total = (int64_t)B * C * (H / 2) * ((W / 2 + 3) / 4);
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return HAV_EUNSUP;
    const bool vec = (W % 8) == 0 && ((((uintptr_t)out) | ((uintptr_t)in)) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(haar_down2_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, out, in, ki4x2x2, fir4x4, kd4x2x2,
                           scale, B, C, H, W, total);
    else
        hipLaunchKernelGGL(haar_down2_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, out, in, ki4x2x2, fir4x4, kd4x2x2,
                           scale, B, C, H, W, total);
    HAV_LAUNCH_CHECK();
    return 0;
}
