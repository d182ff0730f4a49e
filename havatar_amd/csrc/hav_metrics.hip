// hav_metrics.hip -- image-quality metrics of an image pair in one pass: mean SSIM (Wang et al. 2004) and the squared-error sum behind PSNR, gfx950.
//
// Definition, per channel: window g = 11 taps of exp(-k^2 / (2 * 1.5^2)), normalised to sum 1, applied separably on VALID windows (the map is
// (H - 10) x (W - 10));  mu = g * x,  s_xx = g * x^2 - mu_x^2,  s_xy = g * xy - mu_x mu_y;  C1 = (0.01 L)^2, C2 = (0.03 L)^2;
//     ssim = ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)),   value = mean over map and channels, per sample
// -- the numbers of skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False) and pytorch-msssim.
//
// The frames this project scores are composited on white: large parts are flat at 1.0, where g * x^2 - mu^2 in float32 cancels (an error of
// 1e-4 on the mean, 3e-4 on the map: DESIGN.md 7.9).  Here the five moments are ACCUMULATED IN FLOAT64: the inputs are float32 or uint8, so
// x^2, y^2, xy are exact in float64, and what is left is the rounding of 2 x 11 float64 fused multiply-adds per moment (1e-16) against
// C2 = 9e-4 L^2.  No pivot is needed.  The float64 work is 127 fused multiply-adds per output, 0.4 G at 1024^2 x 3; with the float64 LDS traffic
// between the passes it is what the kernel's time goes to (43 us at 1024^2 x 3, a tenth of the memory rate: DESIGN.md 7.9), not its loads.
//
//   metrics_tile_kernel   a 256-thread workgroup owns a MET_TH x MET_TW (32 x 32) tile of the map of one (sample, channel):
//                         1. the haloed 42 x 42 tile of both images goes to the LDS once, row-wise (16-byte loads when W % 4 == 0 and the
//                            images are 16-byte aligned, 4-byte ones otherwise, bytes for the channels-last uint8 form); on the way each
//                            pixel's squared error is added -- a pixel belongs to the tile whose 32 x 32 origin block holds it, the last
//                            tile of a row / column also owns the 10-pixel rim, so every pixel of the image is counted exactly once;
//                         2. horizontal pass: a thread forms 4 neighbouring outputs of one row from 14 staged values, five moments each,
//                            into a float64 LDS array [5][42][32];
//                         3. vertical pass: a thread forms 4 outputs of one column from 14 rows of that array, evaluates the quotient in
//                            float64 (no contraction: identical images give exactly 1), optionally writes the map;
//                         4. two float64 sums of the workgroup (ssim, squared error): wave shuffle tree, then its four waves ascending.
//   metrics_final_kernel  one workgroup per sample adds that sample's records in a fixed order and divides.
// No atomics, no allocation, no synchronisation: the same inputs give the same bits, and the launches can be captured.
//
// LDS: 2 x 42 x 45 floats (row stride 45: the horizontal pass's 8 x 4 lanes of a half-wave fall on 32 distinct banks) + 5 x 42 x 32 doubles
// = 68.9 KB, two workgroups per compute unit.  The vertical pass reads consecutive doubles across the half-wave (conflict-free ds_read_b64).
#include "hav_common.h"

#include <cmath>
#include <type_traits>

#define MET_TH 32
#define MET_TW 32
#define MET_K 11
#define MET_IH (MET_TH + MET_K - 1)          // 42 staged rows
#define MET_IW 44                            // staged columns: 42 needed, 11 16-byte loads
#define MET_LD 45
#define MET_RUN 4                            // outputs per thread and pass
#define MET_TAPS (MET_RUN + MET_K - 1)       // 14 inputs behind them

struct MetWindow { double g[MET_K]; };

// two sums of the workgroup -> dst[0..1], in a fixed order (s2l_block_sums of hav_s2_loss.hip for two values)
__device__ __forceinline__ void met_block_sums(double (&s)[2], double* __restrict__ dst)
{
    __shared__ double sm[4][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_down(s[j], off, HAV_WAVE);
    const int lane = threadIdx.x & (HAV_WAVE - 1), wave = threadIdx.x >> 6;
    if (lane == 0) { sm[wave][0] = s[0]; sm[wave][1] = s[1]; }
    __syncthreads();
    if (threadIdx.x < 2) dst[threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// the quotient; every product and sum rounded on its own, so that x == y gives numerator == denominator bit for bit
__device__ __forceinline__ double met_quotient(double mx, double my, double exx, double eyy, double exy, double C1, double C2)
{
#pragma clang fp contract(off)
    const double mxx = mx * mx, myy = my * my, mxy = mx * my;
    const double sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    const double num = (2.0 * mxy + C1) * (2.0 * sxy + C2);
    const double den = ((mxx + myy) + C1) * ((sxx + syy) + C2);
    return num / den;
}

// T = float: a, b [B,C,H,W] contiguous.  T = uint8_t: [B,H,W,3] channels-last (C == 3), values taken as 0..255.
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) metrics_tile_kernel(double* __restrict__ partials, float* __restrict__ map, const T* __restrict__ a,
                                                           const T* __restrict__ b, int C, int H, int W, int tiles_x, int tiles_y,
                                                           MetWindow win, double C1, double C2)
{
    constexpr bool U8 = std::is_same<T, uint8_t>::value;
    __shared__ float sA[MET_IH * MET_LD], sB[MET_IH * MET_LD];
    __shared__ double sH[5][MET_IH][MET_TW];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int tx = (int)(bid % tiles_x);
    const int64_t t = bid / tiles_x;
    const int ty = (int)(t % tiles_y);
    const int64_t n = t / tiles_y;          // sample * C + channel
    const int OH = H - (MET_K - 1), OW = W - (MET_K - 1);
    const int x0 = tx * MET_TW, y0 = ty * MET_TH;
    const int out_h = min(MET_TH, OH - y0), out_w = min(MET_TW, OW - x0);
    const int in_h = out_h + MET_K - 1, in_w = out_w + MET_K - 1;          // y0 + in_h <= H, x0 + in_w <= W
    const int own_h = ty == tiles_y - 1 ? in_h : MET_TH, own_w = tx == tiles_x - 1 ? in_w : MET_TW;
    const int64_t HW = (int64_t)H * W;
    const int64_t base = U8 ? (n / C) * HW * C + (n % C) : n * HW;          // + (y W + x) * ps
    constexpr int ps = U8 ? 3 : 1;
    double s[2] = {0., 0.};

    // 1. stage the haloed tile; entries outside the image are zero (they reach only outputs that are never used)
    if constexpr (VEC) {
        for (int i = tid; i < MET_IH * (MET_IW / 4); i += 256) {
            const int ly = i / (MET_IW / 4), lx = 4 * (i % (MET_IW / 4));
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (ly < in_h && x0 + lx < W) {          // W % 4 == 0 and x0 % 4 == 0: the four columns are inside together
                const int64_t o = base + (int64_t)(y0 + ly) * W + x0 + lx;
                va = *reinterpret_cast<const float4*>(a + o);
                vb = *reinterpret_cast<const float4*>(b + o);
            }
            const float ea[4] = {va.x, va.y, va.z, va.w}, eb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sA[ly * MET_LD + lx + q] = ea[q];
                sB[ly * MET_LD + lx + q] = eb[q];
                if (ly < own_h && lx + q < own_w) {
                    const double d = (double)ea[q] - (double)eb[q];          // exact
                    s[1] += d * d;
                }
            }
        }
    } else {
        for (int i = tid; i < MET_IH * MET_IW; i += 256) {
            const int ly = i / MET_IW, lx = i % MET_IW;
            float va = 0.f, vb = 0.f;
            if (ly < in_h && lx < in_w) {
                const int64_t o = base + ((int64_t)(y0 + ly) * W + x0 + lx) * ps;
                va = (float)a[o];
                vb = (float)b[o];
            }
            sA[ly * MET_LD + lx] = va;
            sB[ly * MET_LD + lx] = vb;
            if (ly < own_h && lx < own_w) {
                const double d = (double)va - (double)vb;          // exact (uint8: an integer, and so is its square)
                s[1] += d * d;
            }
        }
    }
    __syncthreads();

    // 2. horizontal pass: item = (row, group of 4 columns), the group index fastest across lanes
    for (int it = tid; it < MET_IH * (MET_TW / MET_RUN); it += 256) {
        const int row = it / (MET_TW / MET_RUN), xg = it % (MET_TW / MET_RUN);
        const float* ra = sA + row * MET_LD + MET_RUN * xg;
        const float* rb = sB + row * MET_LD + MET_RUN * xg;
        double acc[5][MET_RUN];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < MET_RUN; ++j) acc[q][j] = 0.;
#pragma unroll
        for (int i = 0; i < MET_TAPS; ++i) {
            const double x = (double)ra[i], y = (double)rb[i];
            const double xx = x * x, yy = y * y, xy = x * y;          // exact: 24-bit significands
#pragma unroll
            for (int j = 0; j < MET_RUN; ++j) {
                const int k = i - j;
                if (k >= 0 && k < MET_K) {
                    const double g = win.g[k];
                    acc[0][j] = fma(g, x, acc[0][j]);
                    acc[1][j] = fma(g, y, acc[1][j]);
                    acc[2][j] = fma(g, xx, acc[2][j]);
                    acc[3][j] = fma(g, yy, acc[3][j]);
                    acc[4][j] = fma(g, xy, acc[4][j]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < MET_RUN; ++j) sH[q][row][MET_RUN * xg + j] = acc[q][j];
    }
    __syncthreads();

    // 3. vertical pass: thread = (column, group of 4 rows)
    {
        const int x = tid % MET_TW, yg = tid / MET_TW;
        double acc[5][MET_RUN];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < MET_RUN; ++j) acc[q][j] = 0.;
#pragma unroll
        for (int i = 0; i < MET_TAPS; ++i) {
            double v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] = sH[q][MET_RUN * yg + i][x];
#pragma unroll
            for (int j = 0; j < MET_RUN; ++j) {
                const int k = i - j;
                if (k >= 0 && k < MET_K) {
                    const double g = win.g[k];
#pragma unroll
                    for (int q = 0; q < 5; ++q) acc[q][j] = fma(g, v[q], acc[q][j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < MET_RUN; ++j) {
            const int y = MET_RUN * yg + j;
            if (y < out_h && x < out_w) {
                const double v = met_quotient(acc[0][j], acc[1][j], acc[2][j], acc[3][j], acc[4][j], C1, C2);
                s[0] += v;
                if (map) map[(n * OH + y0 + y) * (int64_t)OW + x0 + x] = (float)v;
            }
        }
    }
    met_block_sums(s, partials + bid * 2);
}

// workgroup = sample: thread t adds records t, t + 256, ... in ascending order, then the workgroup's fixed tree
__global__ void __launch_bounds__(256) metrics_final_kernel(float* __restrict__ out, const double* __restrict__ partials, int64_t per_sample,
                                                            double n_map, double n_px)
{
    __shared__ double tot[2];
    const double* p = partials + (int64_t)blockIdx.x * per_sample * 2;
    double s[2] = {0., 0.};
    for (int64_t i = threadIdx.x; i < per_sample; i += 256) { s[0] += p[2 * i]; s[1] += p[2 * i + 1]; }
    met_block_sums(s, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        out[2 * (int64_t)blockIdx.x] = (float)(tot[0] / n_map);
        out[2 * (int64_t)blockIdx.x + 1] = (float)(tot[1] / n_px);
    }
}

// workgroups of the tile kernel, 0 where the sizes are refused
static int64_t met_workgroups(int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < MET_K || W < MET_K) return 0;
    const int64_t tiles = (int64_t)((H - MET_K + MET_TH) / MET_TH) * ((W - MET_K + MET_TW) / MET_TW);
    if (tiles > 0x7fffffffLL / ((int64_t)B * C)) return 0;
    return (int64_t)B * C * tiles;
}

static MetWindow met_window()
{
    MetWindow w;
    double sum = 0.;
    for (int k = 0; k < MET_K; ++k) {
        const double d = (double)(k - MET_K / 2);
        w.g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += w.g[k];
    }
    for (int k = 0; k < MET_K; ++k) w.g[k] /= sum;
    return w;
}

extern "C" int64_t hav_image_metrics_blocks(int B, int C, int H, int W) { return 2 * met_workgroups(B, C, H, W); }

template <typename T>
static int met_launch(float* out, double* partials, float* map, const T* a, const T* b, int B, int C, int H, int W, double L, double mse_unit,
                      hipStream_t stream)
{
    if (!out || !partials || !a || !b || B < 1 || C < 1 || H < 1 || W < 1 || !(L > 0.) || !std::isfinite(L)) return HAV_EINVAL;
    const int64_t blocks = met_workgroups(B, C, H, W);
    if (blocks == 0) return HAV_EUNSUP;          // H < 11, W < 11, or a grid beyond 2^31
    const int tiles_x = (W - MET_K + MET_TW) / MET_TW, tiles_y = (H - MET_K + MET_TH) / MET_TH;
    const MetWindow win = met_window();
    const double C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    bool vec = false;
    if constexpr (std::is_same<T, float>::value) vec = (W % 4) == 0 && ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
    if constexpr (std::is_same<T, float>::value) {
        if (vec)
            hipLaunchKernelGGL((metrics_tile_kernel<float, true>), dim3((unsigned)blocks), dim3(256), 0, stream, partials, map, a, b, C, H, W, tiles_x,
                               tiles_y, win, C1, C2);
        else
            hipLaunchKernelGGL((metrics_tile_kernel<float, false>), dim3((unsigned)blocks), dim3(256), 0, stream, partials, map, a, b, C, H, W, tiles_x,
                               tiles_y, win, C1, C2);
    } else {
        hipLaunchKernelGGL((metrics_tile_kernel<uint8_t, false>), dim3((unsigned)blocks), dim3(256), 0, stream, partials, map, a, b, C, H, W, tiles_x,
                           tiles_y, win, C1, C2);
    }
    HAV_LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_final_kernel, dim3((unsigned)B), dim3(256), 0, stream, out, partials, blocks / B,
                       (double)C * (H - MET_K + 1) * (double)(W - MET_K + 1), (double)C * H * (double)W * mse_unit);
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int hav_image_metrics_f32(float* out, double* partials, float* map, const float* a, const float* b, int B, int C, int H, int W,
                                     float data_range, void* stream)
{
    return met_launch<float>(out, partials, map, a, b, B, C, H, W, (double)data_range, 1.0, (hipStream_t)stream);
}

extern "C" int hav_image_metrics_u8(float* out, double* partials, float* map, const uint8_t* a, const uint8_t* b, int B, int H, int W,
                                    void* stream)
{
    return met_launch<uint8_t>(out, partials, map, a, b, B, 3, H, W, 255.0, 255.0 * 255.0, (hipStream_t)stream);
}
