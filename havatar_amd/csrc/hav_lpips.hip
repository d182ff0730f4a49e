// hav_lpips.hip -- the per-tap head of the LPIPS-VGG perceptual loss and the ReLU gradient of its frozen VGG layers, gfx950.
//
// The reference's loss (train_avatar.py:24-29,138-142; train_avatarHD.py:268-274) holds an LPIPS term: two images run through VGG16, and at each of
// five taps the feature maps a, b [B,C,H,W] are compared as
//     a^ = a / (sqrt(sum_c a^2) + 1e-10), b^ likewise;   d[b] = mean_{h,w} sum_c w[c] (a^ - b^)^2
// about a dozen ATen launches per tap each way.  Here:
//   lpips_head_fwd_kernel    two passes over the channels: the norms, then the weighted squared difference of the NORMALISED values (the one-pass
//                            expansion  sum w a^2 / na^2 - 2 sum w a b / (na nb) + sum w b^2 / nb^2  cancels where a ~ b, which is where training
//                            ends up); a workgroup leaves one float64 partial sum
//   lpips_head_final_kernel  one workgroup per sample adds that sample's partials in a fixed order and divides by H W
//   lpips_head_bwd_kernel    with r_k = 2 w_k (a^_k - b^_k) gout[b] / (H W) and n = sqrt(sum a^2):
//                                d/da_c = r_c / (n + eps) - a_c (sum_k r_k a_k) / (n (n + eps)^2)          (for b: r -> -r)
//                            again two passes: the norms and the three weighted sums (sum w a^2, sum w a b, sum w b^2) that give both dot products,
//                            then the write.  The weighted sums are float64 -- products of float32 values are exact there, so the difference
//                            sum w a^2 / (na + eps) - sum w a b / (nb + eps) keeps its digits down to a ~ b and is exactly 0 at a == b.
//                            AT n == 0 THE SECOND TERM IS DROPPED (its limit is 0): the result is finite where differentiating sqrt at 0 gives NaN.
//   relu_mask_*_kernel       gc = g [y > 0], and optionally gbias[c] = sum_{b,p} gc (one workgroup per channel, float64, fixed order)
// No float atomics, no scatter: the same inputs give the same bits on every launch.  No allocation, no synchronisation.
//
// Layout of the head kernels.  A workgroup is 4 waves over the same 64 items; an item is one pixel (any H W, any alignment) or four adjacent
// ones (H W % 4 == 0 and 16-byte aligned maps: 16-byte loads and stores).  Wave w walks the channels w, w + 4, ...: a lane's loads stride by
// H W floats, so every load instruction of a wave is one contiguous run of 256 B (1 KiB) of a channel plane.  The waves' per-pixel sums meet
// in LDS (float64, added in wave order by everyone) between the passes.  The second pass re-reads the tile through the caches: a workgroup's
// tile is 64 (256) pixels x C channels x 2 maps, read again within the few microseconds its first pass took; no LDS staging of the tile
// (at C = 512 it would not fit anyway).
#include "hav_common.h"

#define LP_EPS 1e-10
#define LP_ITEMS 64          // items per workgroup (one per lane; the 4 waves split the channels)

template <int PX> struct lp_vec;
template <> struct lp_vec<1> {
    static __device__ __forceinline__ void load(const float* __restrict__ p, float (&v)[1]) { v[0] = *p; }
    static __device__ __forceinline__ void store(float* __restrict__ p, const float (&v)[1]) { *p = v[0]; }
};
template <> struct lp_vec<4> {
    static __device__ __forceinline__ void load(const float* __restrict__ p, float (&v)[4])
    {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store(float* __restrict__ p, const float (&v)[4])
    {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};

// the four waves' partial sums of NS quantities per pixel -> every wave holds the totals (added in wave order)
template <int NS, int PX>
__device__ __forceinline__ void lp_wave_totals(double (&s)[NS][PX], double (*sm)[NS][PX][LP_ITEMS], int wave, int lane)
{
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int q = 0; q < PX; ++q) sm[wave][j][q][lane] = s[j][q];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int q = 0; q < PX; ++q) s[j][q] = ((sm[0][j][q][lane] + sm[1][j][q][lane]) + sm[2][j][q][lane]) + sm[3][j][q][lane];
}

// one sum of the workgroup -> *dst, in a fixed order: the wave's shuffle tree, then the four waves ascending
__device__ __forceinline__ void lp_block_sum(double s, double* __restrict__ dst)
{
    __shared__ double red[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, HAV_WAVE);
    if ((threadIdx.x & (HAV_WAVE - 1)) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *dst = ((red[0] + red[1]) + red[2]) + red[3];
}

template <int PX>
__global__ void __launch_bounds__(256) lpips_head_fwd_kernel(double* __restrict__ partials, const float* __restrict__ f0, const float* __restrict__ f1,
                                                             const float* __restrict__ w, int C, int64_t HW, int64_t nitems)
{
    __shared__ double sm[4][2][PX][LP_ITEMS];
    const int lane = threadIdx.x & (HAV_WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t item = (int64_t)blockIdx.x * LP_ITEMS + lane;
    const bool valid = item < nitems;
    const int64_t base = (int64_t)blockIdx.y * C * HW + (valid ? item : 0) * PX;
    double s[2][PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) s[0][q] = s[1][q] = 0.;
    if (valid)
        for (int c = wave; c < C; c += 4) {
            float a[PX], b[PX];
            lp_vec<PX>::load(f0 + base + c * HW, a);
            lp_vec<PX>::load(f1 + base + c * HW, b);
#pragma unroll
            for (int q = 0; q < PX; ++q) { s[0][q] += (double)a[q] * (double)a[q]; s[1][q] += (double)b[q] * (double)b[q]; }
        }
    lp_wave_totals<2, PX>(s, sm, wave, lane);
    double acc = 0.;
    if (valid) {
        float ia[PX], ib[PX];
#pragma unroll
        for (int q = 0; q < PX; ++q) { ia[q] = (float)(1. / (sqrt(s[0][q]) + LP_EPS)); ib[q] = (float)(1. / (sqrt(s[1][q]) + LP_EPS)); }
        for (int c = wave; c < C; c += 4) {
            float a[PX], b[PX];
            lp_vec<PX>::load(f0 + base + c * HW, a);
            lp_vec<PX>::load(f1 + base + c * HW, b);
            const float wc = w[c];
#pragma unroll
            for (int q = 0; q < PX; ++q) {
#pragma clang fp contract(off)          // a fused a ia - (b ib) is not 0 at a == b
                const float d = a[q] * ia[q] - b[q] * ib[q];
                acc += (double)(wc * (d * d));
            }
        }
    }
    lp_block_sum(acc, partials + (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// workgroup b: thread t adds partials t, t + 256, ... of sample b in ascending order, then the workgroup's fixed tree
__global__ void __launch_bounds__(256) lpips_head_final_kernel(float* __restrict__ out, const double* __restrict__ partials, int64_t nblk, double inv_hw)
{
    __shared__ double tot;
    const double* p = partials + (int64_t)blockIdx.x * nblk;
    double s = 0.;
    for (int64_t i = threadIdx.x; i < nblk; i += 256) s += p[i];
    lp_block_sum(s, &tot);
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(tot * inv_hw);
}

template <int PX>
__global__ void __launch_bounds__(256) lpips_head_bwd_kernel(float* __restrict__ g0, float* __restrict__ g1, const float* __restrict__ gout,
                                                             const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ w,
                                                             int C, int64_t HW, int64_t nitems, double inv_hw)
{
    __shared__ double sm[4][5][PX][LP_ITEMS];
    const int lane = threadIdx.x & (HAV_WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t item = (int64_t)blockIdx.x * LP_ITEMS + lane;
    const bool valid = item < nitems;
    const int64_t base = (int64_t)blockIdx.y * C * HW + (valid ? item : 0) * PX;
    double s[5][PX];          // sum a^2, sum b^2, sum w a^2, sum w a b, sum w b^2
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int q = 0; q < PX; ++q) s[j][q] = 0.;
    if (valid)
        for (int c = wave; c < C; c += 4) {
            float a[PX], b[PX];
            lp_vec<PX>::load(f0 + base + c * HW, a);
            lp_vec<PX>::load(f1 + base + c * HW, b);
            const double wc = (double)w[c];
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                const double ad = (double)a[q], bd = (double)b[q];
                s[0][q] += ad * ad; s[1][q] += bd * bd;
                // (a a, a b and b b are exact in float64; at a == b the three sums are the same bits)
                s[2][q] += wc * (ad * ad); s[3][q] += wc * (ad * bd); s[4][q] += wc * (bd * bd);
            }
        }
    lp_wave_totals<5, PX>(s, sm, wave, lane);
    if (!valid) return;
    const double k = 2. * (double)gout[blockIdx.y] * inv_hw;
    float ia[PX], ib[PX], ca[PX], cb[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) {
#pragma clang fp contract(off)          // the differences below are exactly 0 at a == b only as products rounded the same way
        const double na = sqrt(s[0][q]), nb = sqrt(s[1][q]);
        const double ja = 1. / (na + LP_EPS), jb = 1. / (nb + LP_EPS);
        const double dot_a = k * (s[2][q] * ja - s[3][q] * jb);          // sum_k r_k a_k
        const double dot_b = -k * (s[3][q] * ja - s[4][q] * jb);         // sum_k (-r_k) b_k
        ia[q] = (float)ja; ib[q] = (float)jb;
        ca[q] = na > 0. ? (float)(dot_a * ja * ja / na) : 0.f;           // n == 0: the term's limit
        cb[q] = nb > 0. ? (float)(dot_b * jb * jb / nb) : 0.f;
    }
    const float kf = (float)k;
    for (int c = wave; c < C; c += 4) {
        float a[PX], b[PX], oa[PX], ob[PX];
        lp_vec<PX>::load(f0 + base + c * HW, a);
        lp_vec<PX>::load(f1 + base + c * HW, b);
        const float wk = w[c] * kf;
#pragma unroll
        for (int q = 0; q < PX; ++q) {
#pragma clang fp contract(off)
            const float r = wk * (a[q] * ia[q] - b[q] * ib[q]);
            oa[q] = r * ia[q] - a[q] * ca[q];
            ob[q] = -r * ib[q] - b[q] * cb[q];
        }
        if (g0) lp_vec<PX>::store(g0 + base + c * HW, oa);
        if (g1) lp_vec<PX>::store(g1 + base + c * HW, ob);
    }
}

template <int PX>
__global__ void __launch_bounds__(256) relu_mask_kernel(float* __restrict__ gc, const float* __restrict__ g, const float* __restrict__ y, int64_t nitems)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nitems) return;
    float gv[PX], yv[PX], o[PX];
    lp_vec<PX>::load(g + i * PX, gv);
    lp_vec<PX>::load(y + i * PX, yv);
#pragma unroll
    for (int q = 0; q < PX; ++q) o[q] = yv[q] > 0.f ? gv[q] : 0.f;
    lp_vec<PX>::store(gc + i * PX, o);
}

// workgroup c: every (b, p) of channel c, thread t the elements t, t + 256, ... of each sample's plane
__global__ void __launch_bounds__(256) relu_mask_bias_kernel(float* __restrict__ gc, float* __restrict__ gbias, const float* __restrict__ g,
                                                             const float* __restrict__ y, int B, int C, int64_t HW)
{
    __shared__ double tot;
    double s = 0.;
    for (int b = 0; b < B; ++b) {
        const int64_t base = ((int64_t)b * C + blockIdx.x) * HW;
        for (int64_t p = threadIdx.x; p < HW; p += 256) {
            const float v = y[base + p] > 0.f ? g[base + p] : 0.f;
            gc[base + p] = v;
            s += (double)v;
        }
    }
    lp_block_sum(s, &tot);
    __syncthreads();
    if (threadIdx.x == 0) gbias[blockIdx.x] = (float)tot;
}

static bool lp_sizes_ok(int B, int C, int H, int W) { return B >= 1 && C >= 1 && H >= 1 && W >= 1; }
static bool lp_aligned16(const void* a, const void* b, const void* c, const void* d)
{
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

extern "C" int64_t hav_lpips_head_blocks(int B, int C, int H, int W)
{
    if (!lp_sizes_ok(B, C, H, W)) return 0;
    return (int64_t)B * (((int64_t)H * W + LP_ITEMS - 1) / LP_ITEMS);          // the one-pixel items' count: the four-pixel path uses fewer
}

extern "C" int hav_lpips_head_fwd(float* out, double* partials, const float* f0, const float* f1, const float* w, int B, int C, int H, int W,
                                  void* stream)
{
    if (!out || !partials || !f0 || !f1 || !w || !lp_sizes_ok(B, C, H, W)) return HAV_EINVAL;
    const int64_t HW = (int64_t)H * W;
    const bool vec = (HW % 4) == 0 && lp_aligned16(f0, f1, nullptr, nullptr);
    const int64_t nitems = vec ? HW / 4 : HW, nblk = (nitems + LP_ITEMS - 1) / LP_ITEMS;
    if (B > 65535 || nblk > 0x7fffffffLL || (int64_t)B * C * HW >= (1LL << 40)) return HAV_EUNSUP;
    const dim3 grid((unsigned)nblk, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(lpips_head_fwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, partials, f0, f1, w, C, HW, nitems);
    else
        hipLaunchKernelGGL(lpips_head_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, partials, f0, f1, w, C, HW, nitems);
    HAV_LAUNCH_CHECK();
    hipLaunchKernelGGL(lpips_head_final_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, out, partials, nblk, 1. / (double)HW);
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int hav_lpips_head_bwd(float* g0, float* g1, const float* gout, const float* f0, const float* f1, const float* w, int B, int C, int H,
                                  int W, void* stream)
{
    if ((!g0 && !g1) || !gout || !f0 || !f1 || !w || !lp_sizes_ok(B, C, H, W)) return HAV_EINVAL;
    const int64_t HW = (int64_t)H * W;
    const bool vec = (HW % 4) == 0 && lp_aligned16(f0, f1, g0, g1);
    const int64_t nitems = vec ? HW / 4 : HW, nblk = (nitems + LP_ITEMS - 1) / LP_ITEMS;
    if (B > 65535 || nblk > 0x7fffffffLL || (int64_t)B * C * HW >= (1LL << 40)) return HAV_EUNSUP;
    const dim3 grid((unsigned)nblk, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(lpips_head_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, g0, g1, gout, f0, f1, w, C, HW, nitems, 1. / (double)HW);
    else
        hipLaunchKernelGGL(lpips_head_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, g0, g1, gout, f0, f1, w, C, HW, nitems, 1. / (double)HW);
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int hav_relu_mask_bwd(float* gc, float* gbias, const float* g, const float* y, int B, int C, int64_t HW, void* stream)
{
    if (!gc || !g || !y || B < 1 || C < 1 || HW < 1) return HAV_EINVAL;
    const int64_t n = (int64_t)B * C * HW;
    if (n >= (1LL << 40)) return HAV_EUNSUP;
    if (gbias) {
        hipLaunchKernelGGL(relu_mask_bias_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, gc, gbias, g, y, B, C, HW);
        HAV_LAUNCH_CHECK();
        return 0;
    }
    const bool vec = (n % 4) == 0 && lp_aligned16(gc, g, y, nullptr);
    const int64_t nitems = vec ? n / 4 : n, blocks = (nitems + 255) / 256;
    if (blocks > 0x7fffffffLL) return HAV_EUNSUP;
    if (vec)
        hipLaunchKernelGGL(relu_mask_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, gc, g, y, nitems);
    else
        hipLaunchKernelGGL(relu_mask_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, gc, g, y, nitems);
    HAV_LAUNCH_CHECK();
    return 0;
}
