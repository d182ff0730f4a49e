// hav_s2_loss.hip -- the image-space losses of the stage-two (HD) joint step as one pass each way, gfx950.
//
// The reference's generator step (train_avatarHD.py:246-283) forms, from the low-resolution render [B,C,r,r] (channels 0..2 are the colour), the
// opacity mask [B,1,r,r] and the generator's image [B,3,G,G]:
//     lr_img   = interpolate(render[:, :3], (G, G), bilinear, align_corners=True)                 :246
//     rgb_loss = l1 | mse (lr_img, gt_lr_img)                                                     :247
//     mask_bce = binary_cross_entropy(mask.clip(1e-3, 1 - 1e-3), gt_lr_mask)                      :251
//     hr_l1    = l1(fake_img, gt_hr_img)                                                          :268
//     mse(lr_img, gt_lr_img), mse(fake_img, gt_hr_img) for the two PSNRs                          :282-283
// about 25 small launches forward and backward, the up-sampling's backward with float atomics.  Here:
//   s2_loss_fwd_kernel   one pass over gt_lr_img, fake_img, gt_hr_img and gt_lr_mask; lr_img is formed in registers and never written; a
//                        workgroup leaves five partial sums in float64 (sum |lr - gt_lr|, sum (lr - gt_lr)^2, sum |fake - gt|, sum (fake - gt)^2, sum bce)
//   s2_loss_final_kernel one workgroup adds the partials in a fixed order and divides by the element counts
//   s2_loss_bwd_kernel   grad_fake and grad_mask elementwise; grad_render as a gather: a thread per low-resolution element walks the
//                        high-resolution pixels whose taps include it and recomputes the residual there
// No float atomics, no scatter: the same inputs give the same bits on every launch.  render / mask (and grad_render) are addressed through
// element strides: the Trainer hands them out as permuted views of [B, r, r, C], and no contiguous copy of the C channels is made.
//
// The bilinear sample repeats ATen's arithmetic (UpSampleBilinear2d.cu, align_corners): scale = (r - 1) / (G - 1) in float, src = scale * dst,
// i0 = int(src), l1 = src - i0, l0 = 1 - l1, the + 1 neighbour clamped at the edge, l0h (l0w a + l1w b) + l1h (l0w c + l1w d).
// The cross entropy is ATen's (Loss.cu): (t - 1) max(log1p(-m), -100) - t max(log(m), -100); its gradient (m - t) / max((1 - m) m, 1e-12), and
// zero where the clip cut (clamp passes the gradient on lo <= m <= hi).  sign(0) = 0.
//
// A thread owns 4 columns of one (b, c, row) of the G x G maps (16-byte loads where G % 4 == 0 and the tensors are 16-byte aligned, 4-byte
// ones otherwise: the kernels are templates on it) and up to 4 mask elements.  256-thread workgroups, one item per thread, no grid cap; the sums
// are float64 (the residuals are float32 like ATen's; adding them up costs no further rounding) and go through the wave (shuffles) before the
// workgroup's LDS step.  No allocation and no synchronisation: the launches can be captured.
//
// Cost of the gather: a low-resolution thread walks (2 (G - 1) / (r - 1) + 4)^2 high-resolution pixels, serially.  At the ratios the harness
// uses (G / r = 4: 12 x 12) that is less than the elementwise part of the same launch; it grows with the square of the ratio while the number
// of threads that share it shrinks, down to r = 2, where 12 B threads each walk a whole G x G map -- correct, but a serial walk: a caller
// with G / r far above 4 and a large G is better served by the ATen statement (HAVATAR_S2_LOSS=0).
#include "hav_common.h"

#define S2L_LO 1e-3f
#define S2L_HI ((float)(1.0 - 1e-3))

// source index pair and weights of output index `dst` (n_in input samples)
__device__ __forceinline__ void s2l_src(float scale, int dst, int n_in, int& i0, int& i1, float& l0, float& l1)
{
    const float src = scale * (float)dst;
    i0 = (int)src;
    if (i0 > n_in - 1) i0 = n_in - 1;          // (never taken for dst < n_out; keeps every address inside the map whatever the rounding)
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

__device__ __forceinline__ float s2l_sample(const float* __restrict__ r0, const float* __restrict__ r1, int64_t o0, int64_t o1,
                                            float l0h, float l1h, float l0w, float l1w)
{
    return l0h * (l0w * r0[o0] + l1w * r0[o1]) + l1h * (l0w * r1[o0] + l1w * r1[o1]);
}

// five sums of the workgroup -> dst[0..4], in a fixed order: the wave's shuffle tree, then its four waves ascending
__device__ __forceinline__ void s2l_block_sums(double (&s)[5], double* __restrict__ dst)
{
    __shared__ double sm[4][5];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_down(s[j], off, HAV_WAVE);
    const int lane = threadIdx.x & (HAV_WAVE - 1), wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) sm[wave][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < 5) dst[threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

template <bool VEC>
__global__ void __launch_bounds__(256) s2_loss_fwd_kernel(double* __restrict__ partials, const float* __restrict__ render, int64_t rsb, int64_t rsc,
                                                          int64_t rsy, int64_t rsx, const float* __restrict__ mask, int64_t msb, int64_t msy,
                                                          int64_t msx, const float* __restrict__ gt_lr, const float* __restrict__ fake,
                                                          const float* __restrict__ gt_hr, const float* __restrict__ gt_mask, int r, int G,
                                                          float scale, int64_t total, int64_t n_mask)
{
    const int G4 = (G + 3) >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s[5] = {0., 0., 0., 0., 0.};
    if (idx < total) {
        const int x4 = (int)(idx % G4);
        const int64_t t = idx / G4;
        const int Y = (int)(t % G);
        const int64_t n = t / G;          // b * 3 + c
        const int64_t b = n / 3, c = n - b * 3;
        int y0, y1;
        float l0h, l1h;
        s2l_src(scale, Y, r, y0, y1, l0h, l1h);
        const float* r0 = render + b * rsb + c * rsc + y0 * rsy;
        const float* r1 = render + b * rsb + c * rsc + y1 * rsy;
        const int64_t off = (n * G + Y) * (int64_t)G + 4 * x4;
        float gl[4], fk[4], gh[4];
        if constexpr (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(gt_lr + off), f = *reinterpret_cast<const float4*>(fake + off),
                         h = *reinterpret_cast<const float4*>(gt_hr + off);
            gl[0] = a.x; gl[1] = a.y; gl[2] = a.z; gl[3] = a.w;
            fk[0] = f.x; fk[1] = f.y; fk[2] = f.z; fk[3] = f.w;
            gh[0] = h.x; gh[1] = h.y; gh[2] = h.z; gh[3] = h.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool ok = 4 * x4 + q < G;
                const int64_t o = ok ? off + q : off;
                gl[q] = gt_lr[o]; fk[q] = fake[o]; gh[q] = gt_hr[o];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int X = 4 * x4 + q;
            const bool ok = VEC || X < G;
            int x0, x1;
            float l0w, l1w;
            s2l_src(scale, ok ? X : G - 1, r, x0, x1, l0w, l1w);
            const float d = s2l_sample(r0, r1, x0 * rsx, x1 * rsx, l0h, l1h, l0w, l1w) - gl[q];
            const float e = fk[q] - gh[q];
            if (ok) { s[0] += (double)fabsf(d); s[1] += (double)d * d; s[2] += (double)fabsf(e); s[3] += (double)e * e; }
        }
    }
    // up to 4 mask elements (n_mask <= 4 total: the launcher checks)
    const int64_t rr = (int64_t)r * r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t m = 4 * idx + q;
        if (m < n_mask) {
            const int64_t b = m / rr, p = m - b * rr;
            const int y = (int)(p / r), x = (int)(p - (int64_t)y * r);
            float v = mask[b * msb + y * msy + x * msx];
            v = fminf(fmaxf(v, S2L_LO), S2L_HI);
            const float t = gt_mask[m];
            s[4] += (double)((t - 1.f) * fmaxf(log1pf(-v), -100.f) - t * fmaxf(logf(v), -100.f));
        }
    }
    s2l_block_sums(s, partials + (int64_t)blockIdx.x * 5);
}

// one workgroup: thread t adds partials t, t + 256, ... in ascending order, then the workgroup's fixed tree; out[j] = sum_j / count_j
__global__ void __launch_bounds__(256) s2_loss_final_kernel(float* __restrict__ out, const double* __restrict__ partials, int64_t nblocks,
                                                            double n_img, double n_mask)
{
    __shared__ double tot[5];
    double s[5] = {0., 0., 0., 0., 0.};
    for (int64_t i = threadIdx.x; i < nblocks; i += 256)
#pragma unroll
        for (int j = 0; j < 5; ++j) s[j] += partials[i * 5 + j];
    s2l_block_sums(s, tot);
    __syncthreads();
    if (threadIdx.x < 5) out[threadIdx.x] = (float)(tot[threadIdx.x] / (threadIdx.x < 4 ? n_img : n_mask));
}

// items: [0, n_fake) 4 columns of grad_fake each; then n_render elements of grad_render; then n_mask elements of grad_mask
template <bool VEC>
__global__ void __launch_bounds__(256) s2_loss_bwd_kernel(float* __restrict__ gfake, float* __restrict__ grender, int64_t gsb, int64_t gsc, int64_t gsy,
                                                          int64_t gsx, float* __restrict__ gmask, const float* __restrict__ gup,
                                                          const float* __restrict__ render, int64_t rsb, int64_t rsc, int64_t rsy, int64_t rsx,
                                                          const float* __restrict__ mask, int64_t msb, int64_t msy, int64_t msx,
                                                          const float* __restrict__ gt_lr, const float* __restrict__ fake,
                                                          const float* __restrict__ gt_hr, const float* __restrict__ gt_mask, int rgb_mse, int r,
                                                          int G, float scale, float inv_scale, float n_img, float n_msk, int64_t n_fake,
                                                          int64_t n_render, int64_t n_mask)
{
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n_fake) {
        const int G4 = (G + 3) >> 2;
        const int x4 = (int)(idx % G4);
        const int64_t row = idx / G4;          // (b * 3 + c) * G + Y
        const int64_t off = row * G + 4 * x4;
        const float k = gup[1] / n_img;
        float o[4];
        if constexpr (VEC) {
            const float4 f = *reinterpret_cast<const float4*>(fake + off), h = *reinterpret_cast<const float4*>(gt_hr + off);
            const float e[4] = {f.x - h.x, f.y - h.y, f.z - h.z, f.w - h.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = e[q] > 0.f ? k : (e[q] < 0.f ? -k : 0.f);
            *reinterpret_cast<float4*>(gfake + off) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (4 * x4 + q < G) {
                    const float e = fake[off + q] - gt_hr[off + q];
                    gfake[off + q] = e > 0.f ? k : (e < 0.f ? -k : 0.f);
                }
        }
        return;
    }
    idx -= n_fake;
    if (idx < n_render) {
        const int xl = (int)(idx % r);
        const int64_t t = idx / r;
        const int yl = (int)(t % r);
        const int64_t n = t / r;          // b * 3 + c
        const int64_t b = n / 3, c = n - b * 3;
        const float* rb = render + b * rsb + c * rsc;
        const float* gb = gt_lr + n * (int64_t)G * G;
        // high-resolution indices whose source lies in (l - 1, l + 1), with a margin for the rounding of the two products; the weights decide
        int Ylo = (int)((float)(yl - 1) * inv_scale) - 1, Yhi = (int)((float)(yl + 1) * inv_scale) + 2;
        int Xlo = (int)((float)(xl - 1) * inv_scale) - 1, Xhi = (int)((float)(xl + 1) * inv_scale) + 2;
        Ylo = Ylo < 0 ? 0 : Ylo; Yhi = Yhi > G - 1 ? G - 1 : Yhi;
        Xlo = Xlo < 0 ? 0 : Xlo; Xhi = Xhi > G - 1 ? G - 1 : Xhi;
        double acc = 0.;
        for (int Y = Ylo; Y <= Yhi; ++Y) {
            int y0, y1;
            float l0h, l1h;
            s2l_src(scale, Y, r, y0, y1, l0h, l1h);
            const float wy = (y0 == yl ? l0h : 0.f) + (y1 == yl ? l1h : 0.f);
            if (y0 != yl && y1 != yl) continue;
            const float* r0 = rb + y0 * rsy;
            const float* r1 = rb + y1 * rsy;
            for (int X = Xlo; X <= Xhi; ++X) {
                int x0, x1;
                float l0w, l1w;
                s2l_src(scale, X, r, x0, x1, l0w, l1w);
                if (x0 != xl && x1 != xl) continue;
                const float wx = (x0 == xl ? l0w : 0.f) + (x1 == xl ? l1w : 0.f);
                const float d = s2l_sample(r0, r1, x0 * rsx, x1 * rsx, l0h, l1h, l0w, l1w) - gb[(int64_t)Y * G + X];
                const float g = rgb_mse ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
                acc += (double)((wy * wx) * g);
            }
        }
        grender[b * gsb + c * gsc + yl * gsy + xl * gsx] = (float)(acc * (double)(gup[0] / n_img));
        return;
    }
    idx -= n_render;
    if (idx < n_mask) {
        const int64_t rr = (int64_t)r * r;
        const int64_t b = idx / rr, p = idx - b * rr;
        const int y = (int)(p / r), x = (int)(p - (int64_t)y * r);
        const float v = mask[b * msb + y * msy + x * msx], t = gt_mask[idx];
        const bool in = v >= S2L_LO && v <= S2L_HI;
        gmask[idx] = in ? ((gup[2] * (v - t)) / fmaxf((1.f - v) * v, 1e-12f)) / n_msk : 0.f;          // ATen's order of the operations (Loss.cu)
    }
}

static bool s2l_sizes_ok(int B, int r, int G) { return B >= 1 && r >= 1 && G >= 1; }

extern "C" int64_t hav_s2_image_loss_blocks(int B, int G)
{
    if (B < 1 || G < 1) return 0;
    const int64_t total = (int64_t)B * 3 * G * ((G + 3) / 4);
    return (total + 255) / 256;
}

extern "C" int hav_s2_image_loss_fwd(float* out5, double* partials, const float* render, int64_t rsb, int64_t rsc, int64_t rsy, int64_t rsx,
                                     const float* mask, int64_t msb, int64_t msy, int64_t msx, const float* gt_lr, const float* fake,
                                     const float* gt_hr, const float* gt_mask, int B, int r, int G, void* stream)
{
    if (!out5 || !partials || !render || !mask || !gt_lr || !fake || !gt_hr || !gt_mask || !s2l_sizes_ok(B, r, G)) return HAV_EINVAL;
    if (r < 2 || r > G) return HAV_EUNSUP;
    const int64_t total = (int64_t)B * 3 * G * ((G + 3) / 4), n_mask = (int64_t)B * r * r;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL || n_mask > 4 * total || (int64_t)B * 3 * G * G >= (1LL << 40)) return HAV_EUNSUP;
    const float scale = (float)(r - 1) / (float)(G - 1);
    const bool vec = (G % 4) == 0 && ((((uintptr_t)gt_lr) | ((uintptr_t)fake) | ((uintptr_t)gt_hr)) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(s2_loss_fwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, partials, render, rsb, rsc, rsy, rsx,
                           mask, msb, msy, msx, gt_lr, fake, gt_hr, gt_mask, r, G, scale, total, n_mask);
    else
        hipLaunchKernelGGL(s2_loss_fwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, partials, render, rsb, rsc, rsy, rsx,
                           mask, msb, msy, msx, gt_lr, fake, gt_hr, gt_mask, r, G, scale, total, n_mask);
    HAV_LAUNCH_CHECK();
    hipLaunchKernelGGL(s2_loss_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out5, partials, blocks, (double)((int64_t)B * 3 * G * G),
                       (double)n_mask);
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int hav_s2_image_loss_bwd(float* gfake, float* grender, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx, float* gmask,
                                     const float* gup3, const float* render, int64_t rsb, int64_t rsc, int64_t rsy, int64_t rsx,
                                     const float* mask, int64_t msb, int64_t msy, int64_t msx, const float* gt_lr, const float* fake,
                                     const float* gt_hr, const float* gt_mask, int rgb_mse, int B, int r, int G, void* stream)
{
    if (!gup3 || !render || !mask || !gt_lr || !fake || !gt_hr || !gt_mask || !s2l_sizes_ok(B, r, G)) return HAV_EINVAL;
    if (r < 2 || r > G) return HAV_EUNSUP;
    const int64_t n_fake = gfake ? (int64_t)B * 3 * G * ((G + 3) / 4) : 0, n_render = grender ? (int64_t)B * 3 * r * r : 0,
                  n_mask = gmask ? (int64_t)B * r * r : 0;
    const int64_t items = n_fake + n_render + n_mask, blocks = (items + 255) / 256;
    if (items == 0) return 0;
    if (blocks > 0x7fffffffLL || (int64_t)B * 3 * G * G >= (1LL << 40)) return HAV_EUNSUP;
    const float scale = (float)(r - 1) / (float)(G - 1), inv_scale = (float)(G - 1) / (float)(r - 1);
    const float n_img = (float)((int64_t)B * 3 * G * G), n_msk = (float)((int64_t)B * r * r);
    const bool vec = (G % 4) == 0 && ((((uintptr_t)gfake) | ((uintptr_t)fake) | ((uintptr_t)gt_hr)) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(s2_loss_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, gfake, grender, gsb, gsc, gsy, gsx, gmask,
                           gup3, render, rsb, rsc, rsy, rsx, mask, msb, msy, msx, gt_lr, fake, gt_hr, gt_mask, rgb_mse, r, G, scale, inv_scale, n_img,
                           n_msk, n_fake, n_render, n_mask);
    else
        hipLaunchKernelGGL(s2_loss_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, gfake, grender, gsb, gsc, gsy, gsx, gmask,
                           gup3, render, rsb, rsc, rsy, rsx, mask, msb, msy, msx, gt_lr, fake, gt_hr, gt_mask, rgb_mse, r, G, scale, inv_scale, n_img,
                           n_msk, n_fake, n_render, n_mask);
    HAV_LAUNCH_CHECK();
    return 0;
}
