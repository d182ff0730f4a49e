// hav_decoder.hip -- what sits between the 3x3x3 convolutions of the skinning-volume decoder (reference model/network/voxel_encoder.py:183-210:
// UpConv3DBlock = ... -> InstanceNorm3d, then the ReLU of :172; :175-178: final_conv -> sigmoid -> cat([s, 1 - s], 1)), forward and
// backward, fp32, NCDHW.  No float atomics anywhere and every sum runs in a fixed order: the same inputs give the same bits.
//
// 1. InstanceNorm3d(affine=False, no running statistics) + ReLU on NC planes of V contiguous floats:
//      z = relu((y - mu) * rstd),  mu = mean(y),  rstd = 1 / sqrt(mean((y - mu)^2) + eps)                      (biased variance)
//      dy = rstd * (gm - mean(gm) - xh * mean(gm * xh)),  xh = (y - mu) * rstd,  gm = dz * [xh > 0]
//    Statistics: a sub-chunk of 4 * NT elements (NT = the threads that own the plane) sits in registers; its mean and then its
//    M2 = sum (y - mean)^2 are tree sums (two passes over registers), and sub-chunks are merged in ascending order by the parallel-variance
//    formula (Chan et al.) -- never sum(y^2) - mean^2.
//    Two forms (hav_inorm_relu_chunks):
//      single owner   one wave (V <= 256) or one workgroup per plane does statistics and apply in one launch;
//      cut            planes of more than 4096 voxels when there are fewer than 2 * CUs of them: a plane is cut into pieces of a multiple
//                     of 1024 voxels, one piece per workgroup.  Three launches: per-piece (mean, M2) or (sum gm, sum gm xh) to the caller's
//                     scratch; one thread per plane merges its pieces in ascending order; the apply pass.  No workgroup waits on another.
//    Grids are capped at IN_CAP * CUs workgroups and walked with a grid stride.  16-byte loads and stores when V % 4 == 0 and the
//    buffers are 16-byte aligned, 4-byte ones otherwise.
//
// 2. The output layer: Conv3d(Cin -> 1, 3x3x3, zero padding 1) + sigmoid + cat([s, 1 - s], 1), direct fp32 arithmetic.
//    Workgroup = 128 threads = a [4 z x 4 y x 32 x] tile of voxels, thread = 4 consecutive x.  The input patch with its halo (6 x 6 x 34) is
//    staged in LDS four channels at a time, the 27 Cin weights sit in LDS; a thread reads a 6-float row segment per (kz, ky) and uses it for
//    4 outputs x 3 taps.
//    Backward: gs = (dvol0 - dvol1) s (1 - s) goes to scratch once (with per-workgroup sums for db);
//      dx[c, p] = sum_t w[c, t] gs[p - off(t)]     the gs patch of a tile sits in 54 registers per thread and serves every channel;
//      dw[c, t] = sum_p x[c, p + off(t)] gs[p]     thread = (channel of the round, tap), walks the tile's 512 voxels out of LDS; a workgroup
//                                                  walks its tiles with a grid stride and keeps the sum in a register; partial sums
//                                                  [workgroup][c][t] are added in workgroup order by the reduce pass, which also adds up db.
#include "hav_common.h"

#define IN_CAP 4                 // workgroups per CU of the capped grids
#define IN_PIECE 1024            // pieces of the cut form are multiples of this
#define IN_OWNER_MAX 4096        // planes up to here always have a single owner
#define IN_WAVE_MAX 256          // ... and up to here that owner is one wave

// ------------------------------------------------------------------------------------------------------------------------------
// sums over the NT threads that own a plane, the same bits in every thread.  NT = 256: one __syncthreads per call, two LDS buffers in turn
// (the barrier of call k + 1 separates the reads of call k from the writes of call k + 2)
template <int NT>
__device__ __forceinline__ float in_sum(float v, float* red, int& flip)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (NT == 64) return v;
    float* r = red + 4 * flip;
    flip ^= 1;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
    __syncthreads();
    return (r[0] + r[1]) + (r[2] + r[3]);
}

// elements [s, s + 4 NT) of a plane, those below hi.  VEC: thread lt holds 4 consecutive ones (hi % 4 == 0), else lt + NT k
template <int NT, bool VEC>
__device__ __forceinline__ void in_load(const float* __restrict__ p, int64_t s, int64_t hi, int lt, float v[4], bool ok[4])
{
    if (VEC) {
        const int64_t i = s + 4 * lt;
        const bool k = i < hi;
        const float4 t = k ? *reinterpret_cast<const float4*>(p + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        ok[0] = ok[1] = ok[2] = ok[3] = k;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = s + lt + NT * k;
            ok[k] = i < hi;
            v[k] = ok[k] ? p[i] : 0.f;
        }
    }
}
template <int NT, bool VEC>
__device__ __forceinline__ void in_store(float* __restrict__ p, int64_t s, int lt, const float v[4], const bool ok[4])
{
    if (VEC) {
        if (ok[0]) *reinterpret_cast<float4*>(p + s + 4 * lt) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k]) p[s + lt + NT * k] = v[k];
    }
}

// (mean, M2) of p[lo, hi)
template <int NT, bool VEC>
__device__ __forceinline__ void in_stats(const float* __restrict__ p, int64_t lo, int64_t hi, int lt, float* red, int& flip, float& mean, float& M2)
{
    float n = 0.f;
    mean = 0.f; M2 = 0.f;
    for (int64_t s = lo; s < hi; s += 4 * NT) {
        float v[4];
        bool ok[4];
        in_load<NT, VEC>(p, s, hi, lt, v, ok);
        const float nc = (float)(hi - s < 4 * NT ? hi - s : 4 * NT);
        const float mc = in_sum<NT>((v[0] + v[1]) + (v[2] + v[3]), red, flip) / nc;          // masked elements are zeros
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float d = ok[k] ? v[k] - mc : 0.f; q += d * d; }
        const float m2c = in_sum<NT>(q, red, flip);
        const float nn = n + nc, delta = mc - mean;
        mean += delta * (nc / nn);
        M2 += m2c + delta * delta * (n * (nc / nn));
        n = nn;
    }
}

template <int NT, bool VEC>
__device__ __forceinline__ void in_apply_fwd(float* __restrict__ z, const float* __restrict__ y, int64_t lo, int64_t hi, int lt, float mu, float r)
{
    for (int64_t s = lo; s < hi; s += 4 * NT) {
        float v[4];
        bool ok[4];
        in_load<NT, VEC>(y, s, hi, lt, v, ok);
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float xh = (v[k] - mu) * r; v[k] = xh < 0.f ? 0.f : xh; }
        in_store<NT, VEC>(z, s, lt, v, ok);
    }
}

// this thread's share of (sum gm, sum gm xh) over [lo, hi)
template <int NT, bool VEC>
__device__ __forceinline__ void in_bwd_sums(const float* __restrict__ dz, const float* __restrict__ y, int64_t lo, int64_t hi, int lt, float mu, float r,
                                            float& s1, float& s2)
{
    s1 = 0.f; s2 = 0.f;
    for (int64_t s = lo; s < hi; s += 4 * NT) {
        float v[4], g[4];
        bool ok[4];
        in_load<NT, VEC>(y, s, hi, lt, v, ok);
        in_load<NT, VEC>(dz, s, hi, lt, g, ok);
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float xh = (v[k] - mu) * r, gm = (ok[k] && xh > 0.f) ? g[k] : 0.f;
            a += gm; b += gm * xh;
        }
        s1 += a; s2 += b;
    }
}

template <int NT, bool VEC>
__device__ __forceinline__ void in_apply_bwd(float* __restrict__ dy, const float* __restrict__ dz, const float* __restrict__ y, int64_t lo, int64_t hi,
                                             int lt, float mu, float r, float m1, float m2)
{
    for (int64_t s = lo; s < hi; s += 4 * NT) {
        float v[4], g[4];
        bool ok[4];
        in_load<NT, VEC>(y, s, hi, lt, v, ok);
        in_load<NT, VEC>(dz, s, hi, lt, g, ok);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float xh = (v[k] - mu) * r, gm = xh > 0.f ? g[k] : 0.f;
            v[k] = r * ((gm - m1) - xh * m2);
        }
        in_store<NT, VEC>(dy, s, lt, v, ok);
    }
}

// single owner: NT threads per plane (a block of 256 holds 256 / NT planes; NT = 64 never meets a barrier: its waves walk different planes)
template <int NT, bool VEC>
__global__ void __launch_bounds__(256) inorm_owner_fwd_kernel(float* __restrict__ z, float* __restrict__ mu, float* __restrict__ rstd, const float* __restrict__ y,
                                                              int64_t NC, int64_t V, float eps)
{
    __shared__ float red[8];
    int flip = 0;
    const int lt = threadIdx.x % NT, grp = threadIdx.x / NT, GPB = 256 / NT;
    for (int64_t pl = (int64_t)blockIdx.x * GPB + grp; pl < NC; pl += (int64_t)gridDim.x * GPB) {
        const float* yp = y + pl * V;
        float mean, M2;
        in_stats<NT, VEC>(yp, 0, V, lt, red, flip, mean, M2);
        const float r = 1.0f / sqrtf(M2 / (float)V + eps);
        if (lt == 0) { mu[pl] = mean; rstd[pl] = r; }
        in_apply_fwd<NT, VEC>(z + pl * V, yp, 0, V, lt, mean, r);
    }
}

template <int NT, bool VEC>
__global__ void __launch_bounds__(256) inorm_owner_bwd_kernel(float* __restrict__ dy, const float* __restrict__ dz, const float* __restrict__ y,
                                                              const float* __restrict__ mu, const float* __restrict__ rstd, int64_t NC, int64_t V)
{
    __shared__ float red[8];
    int flip = 0;
    const int lt = threadIdx.x % NT, grp = threadIdx.x / NT, GPB = 256 / NT;
    for (int64_t pl = (int64_t)blockIdx.x * GPB + grp; pl < NC; pl += (int64_t)gridDim.x * GPB) {
        const float* yp = y + pl * V;
        const float* gp = dz + pl * V;
        const float m = mu[pl], r = rstd[pl];
        float s1, s2;
        in_bwd_sums<NT, VEC>(gp, yp, 0, V, lt, m, r, s1, s2);
        const float m1 = in_sum<NT>(s1, red, flip) / (float)V, m2 = in_sum<NT>(s2, red, flip) / (float)V;
        in_apply_bwd<NT, VEC>(dy + pl * V, gp, yp, 0, V, lt, m, r, m1, m2);
    }
}

// cut form.  item = plane * chunks + piece; piece = [piece * len, min(V, (piece + 1) * len))
template <bool VEC>
__global__ void __launch_bounds__(256) inorm_cut_stats_kernel(float* __restrict__ part, const float* __restrict__ y, int64_t items, int64_t chunks, int64_t len,
                                                              int64_t V)
{
    __shared__ float red[8];
    int flip = 0;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t pl = it / chunks, ck = it - pl * chunks, lo = ck * len, hi = lo + len < V ? lo + len : V;
        float mean, M2;
        in_stats<256, VEC>(y + pl * V, lo, hi, threadIdx.x, red, flip, mean, M2);
        if (threadIdx.x == 0) { part[2 * it] = mean; part[2 * it + 1] = M2; }
    }
}

__global__ void __launch_bounds__(256) inorm_cut_finish_fwd_kernel(float* __restrict__ mu, float* __restrict__ rstd, const float* __restrict__ part, int64_t NC,
                                                                   int64_t chunks, int64_t len, int64_t V, float eps)
{
    const int64_t pl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pl >= NC) return;
    float n = 0.f, mean = 0.f, M2 = 0.f;
    for (int64_t ck = 0; ck < chunks; ++ck) {
        const int64_t lo = ck * len;
        const float nc = (float)(lo + len < V ? len : V - lo), mc = part[2 * (pl * chunks + ck)], m2c = part[2 * (pl * chunks + ck) + 1];
        const float nn = n + nc, delta = mc - mean;
        mean += delta * (nc / nn);
        M2 += m2c + delta * delta * (n * (nc / nn));
        n = nn;
    }
    mu[pl] = mean;
    rstd[pl] = 1.0f / sqrtf(M2 / (float)V + eps);
}

template <bool VEC>
__global__ void __launch_bounds__(256) inorm_cut_apply_fwd_kernel(float* __restrict__ z, const float* __restrict__ y, const float* __restrict__ mu,
                                                                  const float* __restrict__ rstd, int64_t items, int64_t chunks, int64_t len, int64_t V)
{
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t pl = it / chunks, ck = it - pl * chunks, lo = ck * len, hi = lo + len < V ? lo + len : V;
        in_apply_fwd<256, VEC>(z + pl * V, y + pl * V, lo, hi, threadIdx.x, mu[pl], rstd[pl]);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) inorm_cut_sums_kernel(float* __restrict__ part, const float* __restrict__ dz, const float* __restrict__ y,
                                                             const float* __restrict__ mu, const float* __restrict__ rstd, int64_t items, int64_t chunks,
                                                             int64_t len, int64_t V)
{
    __shared__ float red[8];
    int flip = 0;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t pl = it / chunks, ck = it - pl * chunks, lo = ck * len, hi = lo + len < V ? lo + len : V;
        float s1, s2;
        in_bwd_sums<256, VEC>(dz + pl * V, y + pl * V, lo, hi, threadIdx.x, mu[pl], rstd[pl], s1, s2);
        s1 = in_sum<256>(s1, red, flip);
        s2 = in_sum<256>(s2, red, flip);
        if (threadIdx.x == 0) { part[2 * it] = s1; part[2 * it + 1] = s2; }
    }
}

__global__ void __launch_bounds__(256) inorm_cut_finish_bwd_kernel(float* __restrict__ means, const float* __restrict__ part, int64_t NC, int64_t chunks, int64_t V)
{
    const int64_t pl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pl >= NC) return;
    float s1 = 0.f, s2 = 0.f;
    for (int64_t ck = 0; ck < chunks; ++ck) { s1 += part[2 * (pl * chunks + ck)]; s2 += part[2 * (pl * chunks + ck) + 1]; }
    means[2 * pl] = s1 / (float)V;
    means[2 * pl + 1] = s2 / (float)V;
}

template <bool VEC>
__global__ void __launch_bounds__(256) inorm_cut_apply_bwd_kernel(float* __restrict__ dy, const float* __restrict__ dz, const float* __restrict__ y,
                                                                  const float* __restrict__ mu, const float* __restrict__ rstd, const float* __restrict__ means,
                                                                  int64_t items, int64_t chunks, int64_t len, int64_t V)
{
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t pl = it / chunks, ck = it - pl * chunks, lo = ck * len, hi = lo + len < V ? lo + len : V;
        in_apply_bwd<256, VEC>(dy + pl * V, dz + pl * V, y + pl * V, lo, hi, threadIdx.x, mu[pl], rstd[pl], means[2 * pl], means[2 * pl + 1]);
    }
}

static bool in_ok(int64_t NC, int64_t V) { return NC >= 1 && V >= 2 && NC < ((int64_t)1 << 31) && V < ((int64_t)1 << 31); }
// length of a piece (a multiple of IN_PIECE); V: the plane has a single owner
static int64_t in_piece_len(int64_t NC, int64_t V)
{
    const int64_t cus = hav_num_cus();
    if (V <= IN_OWNER_MAX || NC >= 2 * cus) return V;
    int64_t c = (2 * IN_CAP * cus + NC - 1) / NC;          // aim at two pieces per workgroup of the capped grid
    if (c > V / (2 * IN_PIECE)) c = V / (2 * IN_PIECE);
    if (c > 256) c = 256;                                  // the merge of a plane's pieces is one thread's loop
    if (c < 2) return V;
    const int64_t len = ((V + c - 1) / c + IN_PIECE - 1) / IN_PIECE * IN_PIECE;
    return len < V ? len : V;
}
extern "C" int64_t hav_inorm_relu_chunks(int64_t NC, int64_t V)
{
    if (!in_ok(NC, V)) return 0;
    const int64_t len = in_piece_len(NC, V);
    return (V + len - 1) / len;
}
extern "C" int64_t hav_inorm_relu_scratch_bytes(int64_t NC, int64_t V)
{
    const int64_t c = hav_inorm_relu_chunks(NC, V);
    return c > 1 ? (NC * c * 2 + NC * 2) * 4 : 0;
}
static bool in_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static unsigned in_grid(int64_t want) { const int64_t cap = (int64_t)IN_CAP * hav_num_cus(); return (unsigned)(want < cap ? want : cap); }

extern "C" int hav_inorm_relu_fwd(float* z, float* mu, float* rstd, const float* y, int64_t NC, int64_t V, float eps, void* scratch, void* stream)
{
    if (!z || !mu || !rstd || !y || NC < 1 || V < 2 || !(eps >= 0.f)) return HAV_EINVAL;
    if (!in_ok(NC, V)) return HAV_EUNSUP;
    const int64_t len = in_piece_len(NC, V), chunks = (V + len - 1) / len;
    if (chunks > 1 && !scratch) return HAV_EINVAL;
    const bool vec = (V % 4) == 0 && in_aligned16(z) && in_aligned16(y);
    hipStream_t st = (hipStream_t)stream;
    if (chunks == 1) {
        if (V <= IN_WAVE_MAX) {
            const unsigned g = in_grid((NC + 3) / 4);
            if (vec) hipLaunchKernelGGL((inorm_owner_fwd_kernel<64, true>), dim3(g), dim3(256), 0, st, z, mu, rstd, y, NC, V, eps);
            else hipLaunchKernelGGL((inorm_owner_fwd_kernel<64, false>), dim3(g), dim3(256), 0, st, z, mu, rstd, y, NC, V, eps);
        } else {
            const unsigned g = in_grid(NC);
            if (vec) hipLaunchKernelGGL((inorm_owner_fwd_kernel<256, true>), dim3(g), dim3(256), 0, st, z, mu, rstd, y, NC, V, eps);
            else hipLaunchKernelGGL((inorm_owner_fwd_kernel<256, false>), dim3(g), dim3(256), 0, st, z, mu, rstd, y, NC, V, eps);
        }
        HAV_LAUNCH_CHECK();
        return 0;
    }
    float* part = (float*)scratch;
    const int64_t items = NC * chunks;
    const unsigned g = in_grid(items);
    if (vec) hipLaunchKernelGGL(inorm_cut_stats_kernel<true>, dim3(g), dim3(256), 0, st, part, y, items, chunks, len, V);
    else hipLaunchKernelGGL(inorm_cut_stats_kernel<false>, dim3(g), dim3(256), 0, st, part, y, items, chunks, len, V);
    HAV_LAUNCH_CHECK();
    hipLaunchKernelGGL(inorm_cut_finish_fwd_kernel, dim3((unsigned)((NC + 255) / 256)), dim3(256), 0, st, mu, rstd, (const float*)part, NC, chunks, len, V, eps);
    HAV_LAUNCH_CHECK();
    if (vec) hipLaunchKernelGGL(inorm_cut_apply_fwd_kernel<true>, dim3(g), dim3(256), 0, st, z, y, (const float*)mu, (const float*)rstd, items, chunks, len, V);
    else hipLaunchKernelGGL(inorm_cut_apply_fwd_kernel<false>, dim3(g), dim3(256), 0, st, z, y, (const float*)mu, (const float*)rstd, items, chunks, len, V);
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int hav_inorm_relu_bwd(float* dy, const float* dz, const float* y, const float* mu, const float* rstd, int64_t NC, int64_t V, void* scratch,
                                  void* stream)
{
    if (!dy || !dz || !y || !mu || !rstd || NC < 1 || V < 2) return HAV_EINVAL;
    if (!in_ok(NC, V)) return HAV_EUNSUP;
    const int64_t len = in_piece_len(NC, V), chunks = (V + len - 1) / len;
    if (chunks > 1 && !scratch) return HAV_EINVAL;
    const bool vec = (V % 4) == 0 && in_aligned16(dy) && in_aligned16(dz) && in_aligned16(y);
    hipStream_t st = (hipStream_t)stream;
    if (chunks == 1) {
        if (V <= IN_WAVE_MAX) {
            const unsigned g = in_grid((NC + 3) / 4);
            if (vec) hipLaunchKernelGGL((inorm_owner_bwd_kernel<64, true>), dim3(g), dim3(256), 0, st, dy, dz, y, mu, rstd, NC, V);
            else hipLaunchKernelGGL((inorm_owner_bwd_kernel<64, false>), dim3(g), dim3(256), 0, st, dy, dz, y, mu, rstd, NC, V);
        } else {
            const unsigned g = in_grid(NC);
            if (vec) hipLaunchKernelGGL((inorm_owner_bwd_kernel<256, true>), dim3(g), dim3(256), 0, st, dy, dz, y, mu, rstd, NC, V);
            else hipLaunchKernelGGL((inorm_owner_bwd_kernel<256, false>), dim3(g), dim3(256), 0, st, dy, dz, y, mu, rstd, NC, V);
        }
        HAV_LAUNCH_CHECK();
        return 0;
    }
    float* part = (float*)scratch;
    const int64_t items = NC * chunks;
    float* means = part + 2 * items;
    const unsigned g = in_grid(items);
    if (vec) hipLaunchKernelGGL(inorm_cut_sums_kernel<true>, dim3(g), dim3(256), 0, st, part, dz, y, mu, rstd, items, chunks, len, V);
    else hipLaunchKernelGGL(inorm_cut_sums_kernel<false>, dim3(g), dim3(256), 0, st, part, dz, y, mu, rstd, items, chunks, len, V);
    HAV_LAUNCH_CHECK();
    hipLaunchKernelGGL(inorm_cut_finish_bwd_kernel, dim3((unsigned)((NC + 255) / 256)), dim3(256), 0, st, means, (const float*)part, NC, chunks, V);
    HAV_LAUNCH_CHECK();
    if (vec) hipLaunchKernelGGL(inorm_cut_apply_bwd_kernel<true>, dim3(g), dim3(256), 0, st, dy, dz, y, mu, rstd, (const float*)means, items, chunks, len, V);
    else hipLaunchKernelGGL(inorm_cut_apply_bwd_kernel<false>, dim3(g), dim3(256), 0, st, dy, dz, y, mu, rstd, (const float*)means, items, chunks, len, V);
    HAV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The output layer
#define FC_TZ 4
#define FC_TY 4
#define FC_TX 32
#define FC_PD (FC_TZ + 2)
#define FC_PH (FC_TY + 2)
#define FC_PW (FC_TX + 2)
#define FC_ROW 36                               // floats per patch row in LDS: 34 + 2, so that a thread's segment starts 16-byte aligned
#define FC_CH (FC_PD * FC_PH * FC_ROW)          // 1296 floats per staged channel
#define FC_PVOX (FC_PD * FC_PH * FC_PW)         // 1224 voxels of the patch
#define FC_CB 4                                 // channels per round
#define FC_NT 128
#define FC_BATCH 13                             // staging loads in flight per thread: 3 x 13 = the 39 of a four-channel round
#define FC_MAXC 64
#define FC_GS_CAP 4                             // workgroups per CU of the gs pass

struct FcArgs {
    float* out; const float* in; const float* w; const float* bias; float* partial;
    int B, Cin, D, H, W, tz, ty, tx, vec;
    int64_t tiles;
};

__device__ __forceinline__ void fc_tile(const FcArgs& a, int64_t t, int& b, int& z0, int& y0, int& x0)
{
    x0 = (int)(t % a.tx) * FC_TX; t /= a.tx;
    y0 = (int)(t % a.ty) * FC_TY; t /= a.ty;
    z0 = (int)(t % a.tz) * FC_TZ;
    b = (int)(t / a.tz);
}

// CB channels of the patch at (z0 - 1, y0 - 1, x0 - 1) from src (channel stride DHW; channels >= nch and voxels outside the volume: zeros)
template <int CB>
__device__ __forceinline__ void fc_stage(float* __restrict__ lds, const float* __restrict__ src, int nch, int64_t DHW, int z0, int y0, int x0, int D, int H,
                                         int W, int tid)
{
    // loads first (always from a valid address, selected afterwards: no branch between them, so FC_BATCH are in flight), LDS stores after
#pragma unroll 1
    for (int q0 = 0; q0 < (CB * FC_PVOX + FC_NT - 1) / FC_NT; q0 += FC_BATCH) {
        float v[FC_BATCH];
        int dst[FC_BATCH];
#pragma unroll
        for (int u = 0; u < FC_BATCH; ++u) {
            const int e = tid + FC_NT * (q0 + u);
            const bool in = e < CB * FC_PVOX;
            const int ec = in ? e : 0;
            const int cl = ec / FC_PVOX, p = ec - cl * FC_PVOX;
            const int vz = p / (FC_PH * FC_PW), r = p - vz * (FC_PH * FC_PW);
            const int vy = r / FC_PW, vx = r - vy * FC_PW;
            const int gz = z0 + vz - 1, gy = y0 + vy - 1, gx = x0 + vx - 1;
            const bool ok = in && cl < nch && gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const float t = src[ok ? (int64_t)cl * DHW + ((int64_t)gz * H + gy) * W + gx : (int64_t)0];
            v[u] = ok ? t : 0.f;
            dst[u] = in ? cl * FC_CH + (vz * FC_PH + vy) * FC_ROW + vx : -1;
        }
#pragma unroll
        for (int u = 0; u < FC_BATCH; ++u)
            if (dst[u] >= 0) lds[dst[u]] = v[u];
    }
}

__global__ void __launch_bounds__(FC_NT) fc_fwd_kernel(FcArgs a)
{
    __shared__ __attribute__((aligned(16))) float tile[FC_CB * FC_CH];
    __shared__ float wl[FC_MAXC * 27];
    const int tid = threadIdx.x, tz = tid >> 5, ty = (tid >> 3) & 3, xq = tid & 7;
    int b, z0, y0, x0;
    fc_tile(a, blockIdx.x, b, z0, y0, x0);
    const int64_t DHW = (int64_t)a.D * a.H * a.W;
    const int rounds = (a.Cin + FC_CB - 1) / FC_CB;
    for (int i = tid; i < rounds * FC_CB * 27; i += FC_NT) wl[i] = i < a.Cin * 27 ? a.w[i] : 0.f;
    const float* xb = a.in + (int64_t)b * a.Cin * DHW;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < rounds; ++r) {
        __syncthreads();          // the previous round is done with the patch
        fc_stage<FC_CB>(tile, xb + (int64_t)(FC_CB * r) * DHW, a.Cin - FC_CB * r, DHW, z0, y0, x0, a.D, a.H, a.W, tid);
        __syncthreads();
#pragma unroll 1
        for (int cl = 0; cl < FC_CB; ++cl) {
            const float* wc = wl + (FC_CB * r + cl) * 27;
#pragma unroll
            for (int kz = 0; kz < 3; ++kz)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const float* row = tile + cl * FC_CH + ((tz + kz) * FC_PH + ty + ky) * FC_ROW + 4 * xq;
                    const float4 p0 = *reinterpret_cast<const float4*>(row);
                    const float2 p1 = *reinterpret_cast<const float2*>(row + 4);
                    const float v[6] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y};
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float w = wc[kz * 9 + ky * 3 + kx];
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] += w * v[i + kx];
                    }
                }
        }
    }
    const int gz = z0 + tz, gy = y0 + ty, gx = x0 + 4 * xq;
    if (gz >= a.D || gy >= a.H || gx >= a.W) return;
    const float bias = a.bias ? a.bias[0] : 0.f;
    float s[4], c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { s[i] = 1.0f / (1.0f + expf(-(acc[i] + bias))); c[i] = 1.0f - s[i]; }
    float* o0 = a.out + (int64_t)b * 2 * DHW + ((int64_t)gz * a.H + gy) * a.W + gx;
    if (a.vec && gx + 3 < a.W) {
        *reinterpret_cast<float4*>(o0) = make_float4(s[0], s[1], s[2], s[3]);
        *reinterpret_cast<float4*>(o0 + DHW) = make_float4(c[0], c[1], c[2], c[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (gx + i < a.W) { o0[i] = s[i]; o0[DHW + i] = c[i]; }
    }
}

// gs = (dvol0 - dvol1) s (1 - s) over n = B DHW voxels; part[block] = the block's sum of gs (fixed order)
template <bool VEC>
__global__ void __launch_bounds__(256) fc_gs_kernel(float* __restrict__ gs, float* __restrict__ part, const float* __restrict__ dvol, const float* __restrict__ vol,
                                                    int64_t n, int64_t DHW)
{
    __shared__ float red[8];
    int flip = 0;
    float sum = 0.f;
    for (int64_t s = (int64_t)blockIdx.x * 1024; s < n; s += (int64_t)gridDim.x * 1024) {
        if (VEC) {          // DHW % 4 == 0: the four voxels are of one sample
            const int64_t e = s + 4 * threadIdx.x;
            if (e < n) {
                const int64_t b = e / DHW, o = e + b * DHW;          // [B,2,DHW]: channel 0 of sample b starts at 2 b DHW
                const float4 g0 = *reinterpret_cast<const float4*>(dvol + o), g1 = *reinterpret_cast<const float4*>(dvol + o + DHW);
                const float4 sv = *reinterpret_cast<const float4*>(vol + o);
                const float4 r = make_float4((g0.x - g1.x) * sv.x * (1.0f - sv.x), (g0.y - g1.y) * sv.y * (1.0f - sv.y),
                                             (g0.z - g1.z) * sv.z * (1.0f - sv.z), (g0.w - g1.w) * sv.w * (1.0f - sv.w));
                *reinterpret_cast<float4*>(gs + e) = r;
                sum += (r.x + r.y) + (r.z + r.w);
            }
        } else {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t e = s + threadIdx.x + 256 * k;
                if (e < n) {
                    const int64_t b = e / DHW, o = e + b * DHW;
                    const float sv = vol[o], r = (dvol[o] - dvol[o + DHW]) * sv * (1.0f - sv);
                    gs[e] = r;
                    a += r;
                }
            }
            sum += a;
        }
    }
    sum = in_sum<256>(sum, red, flip);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// dx[b, c, p] = sum_t w[c, 26 - t] gs[b, p + off(t)]
__global__ void __launch_bounds__(FC_NT) fc_dx_kernel(FcArgs a)
{
    __shared__ __attribute__((aligned(16))) float tile[FC_CH];
    __shared__ float wl[FC_MAXC * 27];
    const int tid = threadIdx.x, tz = tid >> 5, ty = (tid >> 3) & 3, xq = tid & 7;
    int b, z0, y0, x0;
    fc_tile(a, blockIdx.x, b, z0, y0, x0);
    const int64_t DHW = (int64_t)a.D * a.H * a.W;
    for (int i = tid; i < a.Cin * 27; i += FC_NT) wl[i] = a.w[i];
    fc_stage<1>(tile, a.in + (int64_t)b * DHW, 1, DHW, z0, y0, x0, a.D, a.H, a.W, tid);
    __syncthreads();
    float g[9][6];
#pragma unroll
    for (int kz = 0; kz < 3; ++kz)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const float* row = tile + ((tz + kz) * FC_PH + ty + ky) * FC_ROW + 4 * xq;
            const float4 p0 = *reinterpret_cast<const float4*>(row);
            const float2 p1 = *reinterpret_cast<const float2*>(row + 4);
            float* d = g[kz * 3 + ky];
            d[0] = p0.x; d[1] = p0.y; d[2] = p0.z; d[3] = p0.w; d[4] = p1.x; d[5] = p1.y;
        }
    const int gz = z0 + tz, gy = y0 + ty, gx = x0 + 4 * xq;
    if (gz >= a.D || gy >= a.H || gx >= a.W) return;          // (no barrier below)
    float* o0 = a.out + (int64_t)b * a.Cin * DHW + ((int64_t)gz * a.H + gy) * a.W + gx;
    const bool v4 = a.vec && gx + 3 < a.W;
#pragma unroll 2
    for (int c = 0; c < a.Cin; ++c) {
        const float* wc = wl + c * 27;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float w = wc[26 - (3 * k + kx)];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += w * g[k][i + kx];
            }
        float* o = o0 + (int64_t)c * DHW;
        if (v4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (gx + i < a.W) o[i] = acc[i];
        }
    }
}

// partial[blockIdx.x][c][t] = sum over the workgroup's tiles of sum_p x[c, p + off(t)] gs[p], c in round blockIdx.y.  a.in = x, a.w = gs
__global__ void __launch_bounds__(FC_NT) fc_dw_kernel(FcArgs a)
{
    __shared__ __attribute__((aligned(16))) float tile[FC_CB * FC_CH];
    __shared__ __attribute__((aligned(16))) float gt[FC_TZ * FC_TY * FC_TX];
    const int tid = threadIdx.x, r = blockIdx.y;
    const int cl = tid / 27, t = tid - 27 * cl, kz = t / 9, ky = (t - 9 * kz) / 3, kx = t - 9 * kz - 3 * ky;
    const int64_t DHW = (int64_t)a.D * a.H * a.W;
    float acc = 0.f;
    for (int64_t s = blockIdx.x; s < a.tiles; s += gridDim.x) {
        int b, z0, y0, x0;
        fc_tile(a, s, b, z0, y0, x0);
        __syncthreads();          // the previous tile is done with LDS
        fc_stage<FC_CB>(tile, a.in + ((int64_t)b * a.Cin + FC_CB * r) * DHW, a.Cin - FC_CB * r, DHW, z0, y0, x0, a.D, a.H, a.W, tid);
#pragma unroll
        for (int q = 0; q < FC_TZ * FC_TY * FC_TX / FC_NT; ++q) {
            const int e = tid + FC_NT * q, vz = e >> 7, vy = (e >> 5) & 3, vx = e & 31;
            const int gz = z0 + vz, gy = y0 + vy, gx = x0 + vx;
            const bool ok = gz < a.D && gy < a.H && gx < a.W;
            const float t = a.w[(int64_t)b * DHW + (ok ? ((int64_t)gz * a.H + gy) * a.W + gx : (int64_t)0)];
            gt[e] = ok ? t : 0.f;
        }
        __syncthreads();
        if (cl < FC_CB) {
            float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll 4
            for (int row = 0; row < FC_TZ * FC_TY; ++row) {
                const int vz = row >> 2, vy = row & 3;
                const float* xr = tile + cl * FC_CH + ((vz + kz) * FC_PH + vy + ky) * FC_ROW + kx;
                const float4* gr = reinterpret_cast<const float4*>(gt + row * FC_TX);
#pragma unroll
                for (int j = 0; j < FC_TX / 4; ++j) {
                    const float4 gq = gr[j];
                    t0 += xr[4 * j] * gq.x; t1 += xr[4 * j + 1] * gq.y; t2 += xr[4 * j + 2] * gq.z; t3 += xr[4 * j + 3] * gq.w;
                }
            }
            acc += (t0 + t1) + (t2 + t3);
        }
    }
    const int c = FC_CB * r + cl;
    if (cl < FC_CB && c < a.Cin) a.partial[((int64_t)blockIdx.x * a.Cin + c) * 27 + t] = acc;
}

__global__ void __launch_bounds__(256) fc_reduce_kernel(float* __restrict__ dw, float* __restrict__ db, const float* __restrict__ partial,
                                                        const float* __restrict__ bpart, int G, int GB, int nw)
{
    const int wn = dw ? nw : 0, total = wn + (db ? 1 : 0);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        float s = 0.f;
        if (e < wn) {
            for (int k = 0; k < G; ++k) s += partial[(int64_t)k * nw + e];
            dw[e] = s;
        } else {
            for (int k = 0; k < GB; ++k) s += bpart[k];
            db[0] = s;
        }
    }
}

static bool fc_ok(int B, int Cin, int D, int H, int W)
{
    const int64_t DHW = (int64_t)D * H * W;
    return Cin <= FC_MAXC && (int64_t)Cin * DHW < ((int64_t)1 << 31) && 2 * DHW < ((int64_t)1 << 31) && (int64_t)B * DHW < ((int64_t)1 << 31);          // tiles <= B DHW
}
static void fc_fill(FcArgs& a, int B, int Cin, int D, int H, int W)
{
    a.B = B; a.Cin = Cin; a.D = D; a.H = H; a.W = W;
    a.tz = (D + FC_TZ - 1) / FC_TZ; a.ty = (H + FC_TY - 1) / FC_TY; a.tx = (W + FC_TX - 1) / FC_TX;
    a.tiles = (int64_t)B * a.tz * a.ty * a.tx;
    a.out = nullptr; a.in = nullptr; a.w = nullptr; a.bias = nullptr; a.partial = nullptr; a.vec = 0;
}
static int fc_gs_blocks(int64_t n)
{
    const int64_t want = (n + 1023) / 1024, cap = (int64_t)FC_GS_CAP * hav_num_cus();
    return (int)(want < cap ? want : cap);
}
static int fc_dw_groups(int64_t tiles, int Cin)
{
    const int rounds = (Cin + FC_CB - 1) / FC_CB;
    int64_t g = (2 * (int64_t)hav_num_cus() + rounds - 1) / rounds;          // about two workgroups per CU over all rounds
    if (g > tiles) g = tiles;
    return (int)(g < 1 ? 1 : g);
}

extern "C" int hav_final_conv_sigmoid_fwd(float* vol, const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int D, int H, int W,
                                          void* stream)
{
    if (!vol || !x || !w || B < 1 || Cin < 1 || Cout < 1 || D < 1 || H < 1 || W < 1) return HAV_EINVAL;
    if (Cout != 1 || !fc_ok(B, Cin, D, H, W)) return HAV_EUNSUP;
    FcArgs a;
    fc_fill(a, B, Cin, D, H, W);
    if (a.tiles > 0x7fffffff) return HAV_EUNSUP;
    a.out = vol; a.in = x; a.w = w; a.bias = bias;
    a.vec = (W % 4) == 0 && in_aligned16(vol);
    hipLaunchKernelGGL(fc_fwd_kernel, dim3((unsigned)a.tiles), dim3(FC_NT), 0, (hipStream_t)stream, a);
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t hav_final_conv_sigmoid_bwd_scratch_bytes(int B, int Cin, int Cout, int D, int H, int W)
{
    if (B < 1 || Cin < 1 || Cout != 1 || D < 1 || H < 1 || W < 1 || !fc_ok(B, Cin, D, H, W)) return 0;
    FcArgs a;
    fc_fill(a, B, Cin, D, H, W);
    if (a.tiles > 0x7fffffff) return 0;
    const int64_t n = (int64_t)B * D * H * W, n4 = (n + 3) / 4 * 4;
    return (n4 + fc_gs_blocks(n) + (int64_t)fc_dw_groups(a.tiles, Cin) * Cin * 27) * 4;
}

extern "C" int hav_final_conv_sigmoid_bwd(float* dx, float* dw, float* db, const float* dvol, const float* vol, const float* x, const float* w,
                                          void* scratch, int B, int Cin, int Cout, int D, int H, int W, void* stream)
{
    if ((!dx && !dw && !db) || !dvol || !vol || !scratch || (dw && !x) || (dx && !w) || B < 1 || Cin < 1 || Cout < 1 || D < 1 || H < 1 || W < 1)
        return HAV_EINVAL;
    if (Cout != 1 || !fc_ok(B, Cin, D, H, W)) return HAV_EUNSUP;
    FcArgs a;
    fc_fill(a, B, Cin, D, H, W);
    if (a.tiles > 0x7fffffff) return HAV_EUNSUP;
    hipStream_t st = (hipStream_t)stream;
    const int64_t DHW = (int64_t)D * H * W, n = (int64_t)B * DHW, n4 = (n + 3) / 4 * 4;
    const int GB = fc_gs_blocks(n), G = fc_dw_groups(a.tiles, Cin);
    float* gs = (float*)scratch;
    float* bpart = gs + n4;
    float* partial = bpart + GB;
    if ((DHW % 4) == 0 && in_aligned16(dvol) && in_aligned16(vol) && in_aligned16(gs))
        hipLaunchKernelGGL(fc_gs_kernel<true>, dim3((unsigned)GB), dim3(256), 0, st, gs, bpart, dvol, vol, n, DHW);
    else
        hipLaunchKernelGGL(fc_gs_kernel<false>, dim3((unsigned)GB), dim3(256), 0, st, gs, bpart, dvol, vol, n, DHW);
    HAV_LAUNCH_CHECK();
    if (dx) {
        FcArgs d = a;
        d.out = dx; d.in = gs; d.w = w;
        d.vec = (W % 4) == 0 && in_aligned16(dx);
        hipLaunchKernelGGL(fc_dx_kernel, dim3((unsigned)a.tiles), dim3(FC_NT), 0, st, d);
        HAV_LAUNCH_CHECK();
    }
    if (dw) {
        FcArgs d = a;
        d.in = x; d.w = gs; d.partial = partial;
        hipLaunchKernelGGL(fc_dw_kernel, dim3((unsigned)G, (unsigned)((Cin + FC_CB - 1) / FC_CB)), dim3(FC_NT), 0, st, d);
        HAV_LAUNCH_CHECK();
    }
    if (dw || db) {
        const int nw = Cin * 27;
        hipLaunchKernelGGL(fc_reduce_kernel, dim3((unsigned)((nw + 1 + 255) / 256)), dim3(256), 0, st, dw, db, (const float*)partial, (const float*)bpart, G, GB,
                           nw);
        HAV_LAUNCH_CHECK();
    }
    return 0;
}
