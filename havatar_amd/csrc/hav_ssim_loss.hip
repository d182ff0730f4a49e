// hav_ssim_loss.hip -- the gradient of the mean SSIM of hav_metrics.hip with respect to its first image, gfx950: the backward of the SSIM
// training loss (havatar_amd.metrics.ssim_loss, native/ssim_ops.py).  The forward value is hav_image_metrics_f32's, untouched.
//
// Definition (the header of hav_metrics.hip): 11 taps, sigma 1.5, VALID windows, per channel, the mean over map and channels per sample.
// With the five windowed moments m1, m2, e11, e22, e12 at a map position p (window origin p, taps p .. p + 10),
//     A1 = 2 m1 m2 + C1,  A2 = 2 (e12 - m1 m2) + C2,  B1 = m1^2 + m2^2 + C1,  B2 = (e11 - m1^2) + (e22 - m2^2) + C2,  S = A1 A2 / (B1 B2)
//     D11(p) = dS/de11 = -S / B2          D12(p) = dS/de12 = 2 A1 / (B1 B2)
//     Dm(p)  = dS/dm1  = 2 m2 (A2 - A1) / (B1 B2) + 2 m1 S (1 / B2 - 1 / B1)
//     grad_x[b,c,q] = w_b / (C OH OW) * sum_p g(q_y - p_y) g(q_x - p_x) [ Dm(p) + 2 x_q D11(p) + y_q D12(p) ]
// for L = sum_b w_b ssim_b; the sum over p is the FULL correlation (the adjoint of the valid one): a pixel of the 10-pixel rim is touched by
// fewer windows.  x_q and y_q leave the sum, so three maps are correlated and combined per pixel.
//
// Everything between the float32 loads and the one float32 store is float64, as in the forward and for its reason: on the flat white
// backgrounds e11 - m1^2 cancels in float32, and 1 / B2 (up to 1 / C2 = 1111) carries that error into the gradient.
//
//   ssim_deriv_tile_kernel    a 256-thread workgroup owns a 32 x 32 tile of the MAP of one (sample, channel): the staging and the two
//                             separable float64 passes of metrics_tile_kernel, then Dm, D11, D12 instead of the quotient, written as
//                             float64 into the caller's workspace [3][B,C,OH,OW].
//   ssim_adjoint_tile_kernel  a 256-thread workgroup owns a 32 x 32 tile of PIXELS of one (sample, channel):
//                             1. the 42 x 42 neighbourhood of the three maps (positions q - 10 .. q) goes to the LDS, zeros outside the map;
//                             2. vertical pass: a thread forms 4 rows of one staged column, three maps, into [3][32][42];
//                             3. horizontal pass: a thread forms 4 neighbouring pixels of one row, combines them with x_q, y_q and
//                                w_b / (C OH OW), and stores grad_x -- every pixel once, whatever the buffer held.
//                             16-byte accesses (two doubles of the maps, four floats of x, y, grad_x) when W % 4 == 0 and the pointers are
//                             16-byte aligned, 8- and 4-byte ones otherwise.
// No atomics, no allocation, no synchronisation, no environment reads: the same inputs give the same bits, and the launches can be captured.
//
// LDS: deriv 2 x 42 x 45 floats + 5 x 42 x 32 doubles = 68.9 KB (the forward's); adjoint 3 x 42 x 43 + 3 x 32 x 43 doubles = 76.4 KB (row
// stride 43: the horizontal pass's 8 x 4 lanes of a half-wave read 32 distinct bank pairs with ds_read_b64).  Two workgroups per compute unit.
#include "hav_common.h"

#include <cmath>

#define SSL_T 32                             // tile edge: map elements (deriv), pixels (adjoint)
#define SSL_K 11
#define SSL_I (SSL_T + SSL_K - 1)            // 42 staged rows / columns
#define SSL_IW 44                            // deriv: staged columns, 11 16-byte loads
#define SSL_LD 45                            // deriv: float row stride
#define SSL_DLD 43                           // adjoint: double row stride
#define SSL_RUN 4                            // outputs per thread and pass
#define SSL_TAPS (SSL_RUN + SSL_K - 1)       // 14 inputs behind them

struct SslWindow { double g[SSL_K]; };

// a, b [B,C,H,W] contiguous; ws [3][B*C][OH][OW] receives Dm, D11, D12
template <bool VEC>
__global__ void __launch_bounds__(256) ssim_deriv_tile_kernel(double* __restrict__ ws, const float* __restrict__ a, const float* __restrict__ b,
                                                              int H, int W, int tiles_x, int tiles_y, int64_t plane, SslWindow win, double C1,
                                                              double C2)
{
    __shared__ float sA[SSL_I * SSL_LD], sB[SSL_I * SSL_LD];
    __shared__ double sH[5][SSL_I][SSL_T];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int tx = (int)(bid % tiles_x);
    const int64_t t = bid / tiles_x;
    const int ty = (int)(t % tiles_y);
    const int64_t n = t / tiles_y;          // sample * C + channel
    const int OH = H - (SSL_K - 1), OW = W - (SSL_K - 1);
    const int x0 = tx * SSL_T, y0 = ty * SSL_T;
    const int out_h = min(SSL_T, OH - y0), out_w = min(SSL_T, OW - x0);
    const int in_h = out_h + SSL_K - 1, in_w = out_w + SSL_K - 1;          // y0 + in_h <= H, x0 + in_w <= W
    const int64_t base = n * (int64_t)H * W;

    // 1. stage the haloed tile; entries outside the image are zero (they reach only outputs that are never used)
    if constexpr (VEC) {
        for (int i = tid; i < SSL_I * (SSL_IW / 4); i += 256) {
            const int ly = i / (SSL_IW / 4), lx = 4 * (i % (SSL_IW / 4));
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (ly < in_h && x0 + lx < W) {          // W % 4 == 0 and x0 % 4 == 0: the four columns are inside together
                const int64_t o = base + (int64_t)(y0 + ly) * W + x0 + lx;
                va = *reinterpret_cast<const float4*>(a + o);
                vb = *reinterpret_cast<const float4*>(b + o);
            }
            float* da = sA + ly * SSL_LD + lx;
            float* db = sB + ly * SSL_LD + lx;
            da[0] = va.x; da[1] = va.y; da[2] = va.z; da[3] = va.w;
            db[0] = vb.x; db[1] = vb.y; db[2] = vb.z; db[3] = vb.w;
        }
    } else {
        for (int i = tid; i < SSL_I * SSL_IW; i += 256) {
            const int ly = i / SSL_IW, lx = i % SSL_IW;
            float va = 0.f, vb = 0.f;
            if (ly < in_h && lx < in_w) {
                const int64_t o = base + (int64_t)(y0 + ly) * W + x0 + lx;
                va = a[o];
                vb = b[o];
            }
            sA[ly * SSL_LD + lx] = va;
            sB[ly * SSL_LD + lx] = vb;
        }
    }
    __syncthreads();

    // 2. horizontal pass: item = (row, group of 4 columns), the group index fastest across lanes
    for (int it = tid; it < SSL_I * (SSL_T / SSL_RUN); it += 256) {
        const int row = it / (SSL_T / SSL_RUN), xg = it % (SSL_T / SSL_RUN);
        const float* ra = sA + row * SSL_LD + SSL_RUN * xg;
        const float* rb = sB + row * SSL_LD + SSL_RUN * xg;
        double acc[5][SSL_RUN];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < SSL_RUN; ++j) acc[q][j] = 0.;
#pragma unroll
        for (int i = 0; i < SSL_TAPS; ++i) {
            const double x = (double)ra[i], y = (double)rb[i];
            const double xx = x * x, yy = y * y, xy = x * y;          // exact: 24-bit significands
#pragma unroll
            for (int j = 0; j < SSL_RUN; ++j) {
                const int k = i - j;
                if (k >= 0 && k < SSL_K) {
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
            for (int j = 0; j < SSL_RUN; ++j) sH[q][row][SSL_RUN * xg + j] = acc[q][j];
    }
    __syncthreads();

    // 3. vertical pass: thread = (column, group of 4 rows); then the three derivatives
    const int x = tid % SSL_T, yg = tid / SSL_T;
    double acc[5][SSL_RUN];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int j = 0; j < SSL_RUN; ++j) acc[q][j] = 0.;
#pragma unroll
    for (int i = 0; i < SSL_TAPS; ++i) {
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = sH[q][SSL_RUN * yg + i][x];
#pragma unroll
        for (int j = 0; j < SSL_RUN; ++j) {
            const int k = i - j;
            if (k >= 0 && k < SSL_K) {
                const double g = win.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[q][j] = fma(g, v[q], acc[q][j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < SSL_RUN; ++j) {
        const int y = SSL_RUN * yg + j;
        if (y < out_h && x < out_w) {
            const double m1 = acc[0][j], m2 = acc[1][j], m12 = m1 * m2;
            const double A1 = 2.0 * m12 + C1, A2 = 2.0 * (acc[4][j] - m12) + C2;
            const double B1 = (m1 * m1 + m2 * m2) + C1, B2 = ((acc[2][j] - m1 * m1) + (acc[3][j] - m2 * m2)) + C2;
            const double r1 = 1.0 / B1, r2 = 1.0 / B2, r12 = r1 * r2;
            const double S = (A1 * A2) * r12;
            const int64_t o = (n * OH + y0 + y) * (int64_t)OW + x0 + x;
            ws[o] = 2.0 * m2 * (A2 - A1) * r12 + 2.0 * m1 * S * (r2 - r1);
            ws[plane + o] = -S * r2;
            ws[2 * plane + o] = 2.0 * A1 * r12;
        }
    }
}

// grad, a, b [B,C,H,W] contiguous; ws as written above; wgt [B] = dL/dssim_b
template <bool VEC>
__global__ void __launch_bounds__(256) ssim_adjoint_tile_kernel(float* __restrict__ grad, const double* __restrict__ ws,
                                                                const float* __restrict__ a, const float* __restrict__ b,
                                                                const float* __restrict__ wgt, int C, int H, int W, int tiles_x, int tiles_y,
                                                                int64_t plane, SslWindow win, double inv_count)
{
    __shared__ double sD[3][SSL_I][SSL_DLD];
    __shared__ double sV[3][SSL_T][SSL_DLD];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int tx = (int)(bid % tiles_x);
    const int64_t t = bid / tiles_x;
    const int ty = (int)(t % tiles_y);
    const int64_t n = t / tiles_y;          // sample * C + channel
    const int OH = H - (SSL_K - 1), OW = W - (SSL_K - 1);
    const int qx0 = tx * SSL_T, qy0 = ty * SSL_T;
    const int px0 = qx0 - (SSL_K - 1), py0 = qy0 - (SSL_K - 1);          // the map position behind staged entry (0, 0)

    // 1. stage the three maps at positions (py0 + ly, px0 + lx), zero outside the map
    if constexpr (VEC) {
        // OW is even and px0 is even: the two columns of a pair are inside together, and the pair is 16-byte aligned
        for (int i = tid; i < 3 * SSL_I * (SSL_I / 2); i += 256) {
            const int m = i / (SSL_I * (SSL_I / 2)), r = i % (SSL_I * (SSL_I / 2));
            const int ly = r / (SSL_I / 2), lx = 2 * (r % (SSL_I / 2));
            const int py = py0 + ly, px = px0 + lx;
            double2 v = make_double2(0., 0.);
            if (py >= 0 && py < OH && px >= 0 && px < OW)
                v = *reinterpret_cast<const double2*>(ws + m * plane + (n * OH + py) * (int64_t)OW + px);
            sD[m][ly][lx] = v.x;
            sD[m][ly][lx + 1] = v.y;
        }
    } else {
        for (int i = tid; i < 3 * SSL_I * SSL_I; i += 256) {
            const int m = i / (SSL_I * SSL_I), r = i % (SSL_I * SSL_I);
            const int ly = r / SSL_I, lx = r % SSL_I;
            const int py = py0 + ly, px = px0 + lx;
            double v = 0.;
            if (py >= 0 && py < OH && px >= 0 && px < OW) v = ws[m * plane + (n * OH + py) * (int64_t)OW + px];
            sD[m][ly][lx] = v;
        }
    }
    __syncthreads();

    // 2. vertical pass: item = (group of 4 pixel rows, staged column), the column fastest across lanes.  Pixel row 4 yg + j takes staged
    //    row 4 yg + i with tap q_y - p_y = 10 - (i - j).
    for (int it = tid; it < (SSL_T / SSL_RUN) * SSL_I; it += 256) {
        const int yg = it / SSL_I, lx = it % SSL_I;
        double acc[3][SSL_RUN];
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int j = 0; j < SSL_RUN; ++j) acc[m][j] = 0.;
#pragma unroll
        for (int i = 0; i < SSL_TAPS; ++i) {
            double v[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) v[m] = sD[m][SSL_RUN * yg + i][lx];
#pragma unroll
            for (int j = 0; j < SSL_RUN; ++j) {
                const int k = i - j;
                if (k >= 0 && k < SSL_K) {
                    const double g = win.g[SSL_K - 1 - k];
#pragma unroll
                    for (int m = 0; m < 3; ++m) acc[m][j] = fma(g, v[m], acc[m][j]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int j = 0; j < SSL_RUN; ++j) sV[m][SSL_RUN * yg + j][lx] = acc[m][j];
    }
    __syncthreads();

    // 3. horizontal pass: thread = (pixel row, group of 4 pixel columns), the group index fastest across lanes; combine and store
    const int row = tid / (SSL_T / SSL_RUN), xg = tid % (SSL_T / SSL_RUN);
    const int qy = qy0 + row, qx = qx0 + SSL_RUN * xg;
    if (qy >= H || qx >= W) return;          // (no barrier follows)
    double acc[3][SSL_RUN];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int j = 0; j < SSL_RUN; ++j) acc[m][j] = 0.;
#pragma unroll
    for (int i = 0; i < SSL_TAPS; ++i) {
        double v[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) v[m] = sV[m][row][SSL_RUN * xg + i];
#pragma unroll
        for (int j = 0; j < SSL_RUN; ++j) {
            const int k = i - j;
            if (k >= 0 && k < SSL_K) {
                const double g = win.g[SSL_K - 1 - k];
#pragma unroll
                for (int m = 0; m < 3; ++m) acc[m][j] = fma(g, v[m], acc[m][j]);
            }
        }
    }
    const double scale = (double)wgt[n / C] * inv_count;
    const int64_t o = n * (int64_t)H * W + (int64_t)qy * W + qx;
    if constexpr (VEC) {          // W % 4 == 0: the four pixels are inside together
        const float4 va = *reinterpret_cast<const float4*>(a + o), vb = *reinterpret_cast<const float4*>(b + o);
        const float ea[4] = {va.x, va.y, va.z, va.w}, eb[4] = {vb.x, vb.y, vb.z, vb.w};
        float r[4];
#pragma unroll
        for (int j = 0; j < SSL_RUN; ++j)
            r[j] = (float)(scale * (acc[0][j] + 2.0 * (double)ea[j] * acc[1][j] + (double)eb[j] * acc[2][j]));
        *reinterpret_cast<float4*>(grad + o) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int j = 0; j < SSL_RUN; ++j)
            if (qx + j < W)
                grad[o + j] = (float)(scale * (acc[0][j] + 2.0 * (double)a[o + j] * acc[1][j] + (double)b[o + j] * acc[2][j]));
    }
}

// workgroups of the two launches (map tiles, pixel tiles) per (sample, channel); false where the sizes are refused
static bool ssl_tiles(int B, int C, int H, int W, int64_t* map_tiles, int64_t* px_tiles)
{
    if (B < 1 || C < 1 || H < SSL_K || W < SSL_K) return false;
    *map_tiles = (int64_t)((H - SSL_K + SSL_T) / SSL_T) * ((W - SSL_K + SSL_T) / SSL_T);
    *px_tiles = (int64_t)((H + SSL_T - 1) / SSL_T) * ((W + SSL_T - 1) / SSL_T);          // >= map_tiles
    return *px_tiles <= 0x7fffffffLL / ((int64_t)B * C);
}

static SslWindow ssl_window()          // met_window of hav_metrics.hip
{
    SslWindow w;
    double sum = 0.;
    for (int k = 0; k < SSL_K; ++k) {
        const double d = (double)(k - SSL_K / 2);
        w.g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += w.g[k];
    }
    for (int k = 0; k < SSL_K; ++k) w.g[k] /= sum;
    return w;
}

extern "C" int64_t hav_ssim_grad_blocks(int B, int C, int H, int W)
{
    int64_t mt, pt;
    return ssl_tiles(B, C, H, W, &mt, &pt) ? (int64_t)B * C * (mt + pt) : 0;
}

extern "C" int hav_ssim_loss_bwd_f32(float* grad_x, double* ws, const float* x, const float* y, const float* gout, int B, int C, int H, int W,
                                     float data_range, void* stream_)
{
    const double L = (double)data_range;
    if (!grad_x || !ws || !x || !y || !gout || B < 1 || C < 1 || H < 1 || W < 1 || !(L > 0.) || !std::isfinite(L)) return HAV_EINVAL;
    int64_t mt, pt;
    if (!ssl_tiles(B, C, H, W, &mt, &pt)) return HAV_EUNSUP;          // H < 11, W < 11, or a grid beyond 2^31
    hipStream_t stream = (hipStream_t)stream_;
    const int OH = H - SSL_K + 1, OW = W - SSL_K + 1;
    const int64_t plane = (int64_t)B * C * OH * OW;
    const SslWindow win = ssl_window();
    const double C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    const bool vec = (W % 4) == 0 && ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)grad_x) | ((uintptr_t)ws)) & 15) == 0;
    const int mtx = (W - SSL_K + SSL_T) / SSL_T, mty = (H - SSL_K + SSL_T) / SSL_T;
    const int ptx = (W + SSL_T - 1) / SSL_T, pty = (H + SSL_T - 1) / SSL_T;
    const dim3 gd((unsigned)((int64_t)B * C * mt)), ga((unsigned)((int64_t)B * C * pt));
    if (vec)
        hipLaunchKernelGGL((ssim_deriv_tile_kernel<true>), gd, dim3(256), 0, stream, ws, x, y, H, W, mtx, mty, plane, win, C1, C2);
    else
        hipLaunchKernelGGL((ssim_deriv_tile_kernel<false>), gd, dim3(256), 0, stream, ws, x, y, H, W, mtx, mty, plane, win, C1, C2);
    HAV_LAUNCH_CHECK();
    const double inv_count = 1.0 / ((double)C * OH * (double)OW);
    if (vec)
        hipLaunchKernelGGL((ssim_adjoint_tile_kernel<true>), ga, dim3(256), 0, stream, grad_x, ws, x, y, gout, C, H, W, ptx, pty, plane, win,
                           inv_count);
    else
        hipLaunchKernelGGL((ssim_adjoint_tile_kernel<false>), ga, dim3(256), 0, stream, grad_x, ws, x, y, gout, C, H, W, ptx, pty, plane, win,
                           inv_count);
    HAV_LAUNCH_CHECK();
    return 0;
}
