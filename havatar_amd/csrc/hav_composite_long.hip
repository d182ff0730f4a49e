// hav_composite_long.hip -- compositing with gradients for up to 128 samples per ray: volume_render_radiance_field(act_feat=False) +
// cumprod_exclusive (utils/nerf_util.py:4-73 of the reference), the mathematics of composite_kernel (hav_train.hip, S <= 64):
//   dist_i = (z_{i+1} - z_i) |rd|, the last one repeated (:36-40);  sigma_i = relu(raw_i + noise_i) (:54-58);  alpha_i = 1 - exp(-sigma_i dist_i)
//   (:59);  T_i = prod_{j<i} (1 - alpha_j + 1e-10), w_i = alpha_i T_i (:60);  rgb = sum_i w_i c_i with a sigmoid on the first n_sigmoid
//   channels (:45-46, :62-63), depth = sum_i w_i z_i, acc = sum_i w_i (:64-68);  rgb[:3] += (1 - acc) bg (:70-71).
// One wave per ray, a grid-stride loop over rays, grids capped at a multiple of the CU count -- as there.  What differs:
//   * a lane owns the two adjacent samples 2l, 2l+1 (8-byte loads of z / noise / d_weights where the rows allow it).  The exclusive
//     transmittance product and the suffix sum of G_j w_j stay ONE six-step wave scan each: the lane's own pair is folded before the scan
//     and unfolded after it.  The products are associated as a tree, not in ATen's cumprod order.
//   * the per-wave weight / density-gradient rows hold 128 entries; slots >= S carry alpha = 0, tt = 1, w = 0, G = 0.
//   * the backward stages the ray's S x (CH+1) block in LDS (pitch CH+1 words: 69 at the model's size, odd, so neither the row walk of the
//     lane = sample phase nor the linear walk of the output phase conflicts), overwrites it in place with the gradient block and copies
//     that out as 16-byte vectors.  At 128 x 69 the block is 35 KB: one wave per workgroup fits the 64 KB a kernel gets without asking;
//     the two-wave arrangement raises hipFuncAttributeMaxDynamicSharedMemorySize.  A block larger than one wave may hold takes the form
//     that walks the rows in memory (MODE 1).
//   * the output phase of the backward walks the block linearly (element e = 64 k + lane) instead of one column per lane: with CH+1 = 69
//     columns the column walk leaves 59 lanes idle on its second trip; the linear walk keeps all 64 busy and its stores are contiguous.
// LDS and global pointers live in different `if constexpr` branches: no FLAT access.  No float atomics, no allocation, no
// synchronisation, no environment: the form of the backward is picked by shape (hav_composite_long_bwd) or named by the caller
// (hav_composite_long_bwd_form: the A/B tool and the tests of each form).
#include "hav_common.h"
#include <atomic>

#define CL_MAXS 128

struct CompLongArgs {
    float* rgb; float* acc; float* weights; float* depth;                  // fwd out
    float* d_rf;                                                          // bwd out
    const float* d_rgb; const float* d_acc; const float* d_w; const float* d_depth;
    const float* rf; const float* z; const float* rd; const float* noise; const float* bg;
    int64_t n_rays;
    int S, CH, nsig;
    int vec;          // S even and every per-sample row (z, noise, weights / d_weights) 8-byte aligned: a lane's pair is one 8-byte access
    int pitch;        // MODE 2: floats of dynamic LDS per wave = S (CH+1) + (CH+1), rounded up to a multiple of 4
};

__device__ __forceinline__ float cl_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float cl_wsum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a lane's pair of a per-sample row: samples 2l, 2l+1 (indices clamped to the row for slots >= S, whose values are never used)
__device__ __forceinline__ void cl_load_pair(const float* __restrict__ row, int S, int lane, bool vec, float& v0, float& v1)
{
    if (vec) {
        const int p = min(lane, (S >> 1) - 1);
        const float2 v = reinterpret_cast<const float2*>(row)[p];
        v0 = v.x; v1 = v.y;
    } else {
        v0 = row[min(2 * lane, S - 1)];
        v1 = row[min(2 * lane + 1, S - 1)];
    }
}

// MODE 0: forward.  MODE 1: backward, rows read from memory.  MODE 2: backward, the ray's block staged in LDS.
template <int MODE, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) composite_long_kernel(CompLongArgs a)
{
    __shared__ __attribute__((aligned(16))) float sw_[WAVES][CL_MAXS], sd_[WAVES][CL_MAXS];
    extern __shared__ __attribute__((aligned(16))) float cl_lds[];          // MODE 2: [waves][pitch] = the block [S][RW], then d_rgb [RW]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* sw = sw_[wv]; float* sd = sd_[wv];
    const int S = a.S, CH = a.CH, RW = a.CH + 1, nel = S * RW;
    const bool vec = a.vec != 0;
    const int s0 = 2 * lane, s1 = 2 * lane + 1;
    const bool on0 = s0 < S, on1 = s1 < S;
    const int c0 = min(s0, S - 1), c1 = min(s1, S - 1);
    for (int64_t r = (int64_t)blockIdx.x * WAVES + wv; r < a.n_rays; r += (int64_t)gridDim.x * WAVES) {
        const float* __restrict__ grf = a.rf + (size_t)r * nel;
        float* srf = cl_lds + (size_t)wv * a.pitch;
        if constexpr (MODE == 2) {
            // the lane = sample phase walks two rows of CH + 1 values per lane: from memory that is 128 cache lines per load instruction.
            // The block is copied once, coalesced, into LDS and read there.
            __builtin_amdgcn_wave_barrier();
            if ((nel & 3) == 0 && ((reinterpret_cast<uintptr_t>(grf) & 15) == 0)) {
                const int n4 = nel >> 2;          // 6 vectors per lane in flight
                for (int e0 = 0; e0 < n4; e0 += 6 * 64) {
                    float4 v[6];
#pragma unroll
                    for (int u = 0; u < 6; ++u) { const int e = e0 + 64 * u + lane; v[u] = e < n4 ? reinterpret_cast<const float4*>(grf)[e] : make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
                    for (int u = 0; u < 6; ++u) { const int e = e0 + 64 * u + lane; if (e < n4) reinterpret_cast<float4*>(srf)[e] = v[u]; }
                }
            } else {
                for (int e = lane; e < nel; e += 64) srf[e] = grf[e];
            }
            const float* __restrict__ g = a.d_rgb + (size_t)r * CH;
            for (int c = lane; c < RW; c += 64) srf[nel + c] = c < CH ? g[c] : 0.f;
            __builtin_amdgcn_wave_barrier();
        }
        // ---- lane = sample pair: alpha, transmittance, weight (:36-60)
        float z0, z1, n0 = 0.f, n1 = 0.f, raw0, raw1;
        cl_load_pair(a.z + r * S, S, lane, vec, z0, z1);
        if (a.noise) cl_load_pair(a.noise + r * S, S, lane, vec, n0, n1);
        if constexpr (MODE == 2) { raw0 = srf[c0 * RW + CH]; raw1 = srf[c1 * RW + CH]; }
        else { raw0 = grf[(size_t)c0 * RW + CH]; raw1 = grf[(size_t)c1 * RW + CH]; }
        raw0 += n0; raw1 += n1;
        // the distance to the next sample; the last distance is repeated (:37)
        const float z1n = __shfl_down(z0, 1, 64), z1p = __shfl_up(z1, 1, 64);
        const float dz0 = s0 < S - 1 ? z1 - z0 : (S > 1 ? z0 - z1p : 0.f);
        const float dz1 = s1 < S - 1 ? z1n - z1 : z1 - z0;
        const float dx = a.rd[r * 3], dy = a.rd[r * 3 + 1], dzz = a.rd[r * 3 + 2];
        const float nrm = sqrtf(dx * dx + dy * dy + dzz * dzz);
        const float dist0 = dz0 * nrm, dist1 = dz1 * nrm;
        const float alpha0 = on0 ? 1.0f - expf(-fmaxf(raw0, 0.f) * dist0) : 0.f;
        const float alpha1 = on1 ? 1.0f - expf(-fmaxf(raw1, 0.f) * dist1) : 0.f;
        const float tt0 = on0 ? (1.0f - alpha0) + 1e-10f : 1.0f;
        const float tt1 = on1 ? (1.0f - alpha1) + 1e-10f : 1.0f;
        float incl = tt0 * tt1;          // the pair folded: one scan over 64 lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float u = __shfl_up(incl, o, 64);
            if (lane >= o) incl *= u;
        }
        float excl0 = __shfl_up(incl, 1, 64);
        if (lane == 0) excl0 = 1.0f;
        const float excl1 = excl0 * tt0;          // ... and unfolded
        const float w0 = alpha0 * excl0, w1 = alpha1 * excl1;
        const float acc = cl_wsum(w0 + w1);
        __builtin_amdgcn_wave_barrier();      // sw / sd are private to the wave: LDS executes a wave's accesses in order
        *reinterpret_cast<float2*>(sw + s0) = make_float2(w0, w1);
        if constexpr (MODE == 0) {
            const float depth = cl_wsum(w0 * z0 + w1 * z1);
            float* wr = a.weights + r * S;
            if (vec) { if (on0) reinterpret_cast<float2*>(wr)[lane] = make_float2(w0, w1); }
            else { if (on0) wr[s0] = w0; if (on1) wr[s1] = w1; }
            if (lane == 0) { a.acc[r] = acc; a.depth[r] = depth; }
            __builtin_amdgcn_wave_barrier();
            // ---- lane = channel: rgb_map = sum_i w_i c_i (:62-63), white-background term on the first three (:70-71)
            for (int c = lane; c < CH; c += 64) {
                float s = 0.f;
                for (int i = 0; i < S; ++i) {
                    const float v = grf[(size_t)i * RW + c];
                    s += sw[i] * (c < a.nsig ? cl_sigmoid(v) : v);
                }
                if (a.bg && c < 3) s += (1.0f - acc) * a.bg[r * 3 + c];
                a.rgb[r * CH + c] = s;
            }
        } else {
            // ---- G_i = d loss / d w_i
            const float* __restrict__ drgb = a.d_rgb + (size_t)r * CH;
            float dacc = a.d_acc ? a.d_acc[r] : 0.f;
            if (a.bg)
                for (int c = 0; c < 3 && c < CH; ++c) dacc -= drgb[c] * a.bg[r * 3 + c];
            const float dd = a.d_depth ? a.d_depth[r] : 0.f;
            float dw0 = 0.f, dw1 = 0.f;
            if (a.d_w) cl_load_pair(a.d_w + r * S, S, lane, vec, dw0, dw1);
            float dot0 = 0.f, dot1 = 0.f;
            const int ns = min(a.nsig, CH);
            if constexpr (MODE == 2) {
                const float* row0 = srf + c0 * RW; const float* row1 = srf + c1 * RW; const float* sg = srf + nel;
                for (int c = 0; c < ns; ++c) { const float g = sg[c]; dot0 += g * cl_sigmoid(row0[c]); dot1 += g * cl_sigmoid(row1[c]); }
                for (int c = ns; c < CH; ++c) { const float g = sg[c]; dot0 += g * row0[c]; dot1 += g * row1[c]; }
            } else {
                const float* __restrict__ row0 = grf + (size_t)c0 * RW; const float* __restrict__ row1 = grf + (size_t)c1 * RW;
                for (int c = 0; c < ns; ++c) { const float g = drgb[c]; dot0 += g * cl_sigmoid(row0[c]); dot1 += g * cl_sigmoid(row1[c]); }
                for (int c = ns; c < CH; ++c) { const float g = drgb[c]; dot0 += g * row0[c]; dot1 += g * row1[c]; }
            }
            const float G0 = on0 ? dacc + dd * z0 + dw0 + dot0 : 0.f;
            const float G1 = on1 ? dacc + dd * z1 + dw1 + dot1 : 0.f;
            // suffix sum of G_j w_j over j > i: the pair folded, one scan, the upper sample's term added back for the lower one
            float sufi = G0 * w0 + G1 * w1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float u = __shfl_down(sufi, o, 64);
                if (lane + o < 64) sufi += u;
            }
            float suf1 = __shfl_down(sufi, 1, 64);
            if (lane == 63) suf1 = 0.f;
            const float suf0 = suf1 + G1 * w1;
            const float dsig0 = (G0 * excl0 - suf0 / tt0) * dist0 * (1.0f - alpha0);
            const float dsig1 = (G1 * excl1 - suf1 / tt1) * dist1 * (1.0f - alpha1);
            *reinterpret_cast<float2*>(sd + s0) = make_float2((on0 && raw0 > 0.f) ? dsig0 : 0.f, (on1 && raw1 > 0.f) ? dsig1 : 0.f);
            __builtin_amdgcn_wave_barrier();
            // ---- element e = 64 k + lane of the block: d c_i = w_i d_rgb (sigmoid' on the first nsig), d raw_i in the last column
            float* __restrict__ dst = a.d_rf + (size_t)r * nel;
            int i = lane / RW, c = lane - i * RW;
            const int di = 64 / RW, dc = 64 - di * RW;
            for (int e = lane; e < nel; e += 64) {
                float o;
                if constexpr (MODE == 2) {
                    if (c == CH) o = sd[i];
                    else if (c < a.nsig) { const float sg = cl_sigmoid(srf[e]); o = sw[i] * srf[nel + c] * sg * (1.0f - sg); }
                    else o = sw[i] * srf[nel + c];
                    srf[e] = o;          // the gradient block replaces the staged one in place
                } else {
                    if (c == CH) o = sd[i];
                    else if (c < a.nsig) { const float sg = cl_sigmoid(grf[e]); o = sw[i] * drgb[c] * sg * (1.0f - sg); }
                    else o = sw[i] * drgb[c];
                    dst[e] = o;
                }
                i += di; c += dc;
                if (c >= RW) { c -= RW; ++i; }
            }
            if constexpr (MODE == 2) {          // ... and leaves as whole 16-byte vectors, a contiguous KiB per wave and store
                __builtin_amdgcn_wave_barrier();
                if ((nel & 3) == 0 && ((reinterpret_cast<uintptr_t>(dst) & 15) == 0)) {
                    for (int e = lane; e < (nel >> 2); e += 64) reinterpret_cast<float4*>(dst)[e] = reinterpret_cast<const float4*>(srf)[e];
                } else {
                    for (int e = lane; e < nel; e += 64) dst[e] = srf[e];
                }
            }
        }
    }
}

static bool cl_al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// grids: ceil(rays / waves per workgroup) workgroups, capped at CL_CAP_* per CU
#define CL_CAP_WIDE 16          // forward and direct backward: 4 waves per workgroup
#define CL_CAP_ONE 16           // staged backward, 1 wave per workgroup
#define CL_CAP_TWO 8            // staged backward, 2 waves per workgroup
#define CL_LDS_STATIC (2 * CL_MAXS * (int)sizeof(float))          // sw + sd, per wave
#define CL_LDS_DEFAULT (64 * 1024)          // what a kernel may use without the attribute
#define CL_LDS_MAX (160 * 1024)

static unsigned cl_blocks(int64_t n_rays, int waves, int cap_per_cu)
{
    const int64_t blocks = (n_rays + waves - 1) / waves, cap = (int64_t)hav_num_cus() * cap_per_cu;
    return (unsigned)(blocks > cap ? cap : blocks);
}

extern "C" int hav_composite_long_fwd(float* rgb, float* acc, float* weights, float* depth, const float* rf, const float* z, const float* rd,
                                      const float* noise, const float* bg, int64_t n_rays, int S, int CH, int n_sigmoid, void* stream)
{
    if (n_rays < 0 || S < 1 || CH < 1 || n_sigmoid < 0) return HAV_EINVAL;
    if (S > CL_MAXS) return HAV_EUNSUP;
    if (n_rays == 0) return 0;          // (empty tensors have null pointers)
    if (!rgb || !acc || !weights || !depth || !rf || !z || !rd) return HAV_EINVAL;
    CompLongArgs a{};
    a.rgb = rgb; a.acc = acc; a.weights = weights; a.depth = depth; a.rf = rf; a.z = z; a.rd = rd; a.noise = noise; a.bg = bg;
    a.n_rays = n_rays; a.S = S; a.CH = CH; a.nsig = n_sigmoid;
    a.vec = (S & 1) == 0 && cl_al8(z) && cl_al8(noise) && cl_al8(weights);
    hipLaunchKernelGGL((composite_long_kernel<0, 4>), dim3(cl_blocks(n_rays, 4, CL_CAP_WIDE)), dim3(256), 0, (hipStream_t)stream, a);
    HAV_LAUNCH_CHECK();
    return 0;
}

// form: 0 = by shape (hav_composite_long_bwd), 1 = staged, one wave per workgroup, 2 = staged, two waves per workgroup, 3 = rows from memory
extern "C" int hav_composite_long_bwd_form(float* d_rf, const float* d_rgb, const float* d_acc, const float* d_weights, const float* d_depth,
                                           const float* rf, const float* z, const float* rd, const float* noise, const float* bg,
                                           int64_t n_rays, int S, int CH, int n_sigmoid, int form, void* stream)
{
    if (n_rays < 0 || S < 1 || CH < 1 || n_sigmoid < 0 || form < 0 || form > 3) return HAV_EINVAL;
    if (S > CL_MAXS) return HAV_EUNSUP;
    if (n_rays > 0 && (!d_rf || !d_rgb || !rf || !z || !rd)) return HAV_EINVAL;
    const int64_t pitch = (((int64_t)S * (CH + 1) + (CH + 1)) + 3) & ~(int64_t)3;
    const int64_t lds1 = pitch * 4 + CL_LDS_STATIC, lds2 = 2 * lds1;          // static + dynamic bytes of the two staged arrangements
    // by shape: the one-wave arrangement while a ray's block fits what a kernel gets by default, rows from memory beyond
    // (128 x 69: 36 KB.  8 192 rays, forward + backward: one wave per workgroup 350 / 469 / 614 us at S = 80 / 96 / 128, two waves
    // 358 / 485 / 632 us -- profiles/composite_long_ab.txt)
    if (form == 0) form = lds1 <= CL_LDS_DEFAULT ? 1 : 3;
    if ((form == 1 && lds1 > CL_LDS_DEFAULT) || (form == 2 && lds2 > CL_LDS_MAX)) return HAV_EUNSUP;
    if (n_rays == 0) return 0;
    CompLongArgs a{};
    a.d_rf = d_rf; a.d_rgb = d_rgb; a.d_acc = d_acc; a.d_w = d_weights; a.d_depth = d_depth;
    a.rf = rf; a.z = z; a.rd = rd; a.noise = noise; a.bg = bg;
    a.n_rays = n_rays; a.S = S; a.CH = CH; a.nsig = n_sigmoid; a.pitch = (int)pitch;
    a.vec = (S & 1) == 0 && cl_al8(z) && cl_al8(noise) && cl_al8(d_weights);
    hipStream_t st = (hipStream_t)stream;
    if (form == 1) {
        hipLaunchKernelGGL((composite_long_kernel<2, 1>), dim3(cl_blocks(n_rays, 1, CL_CAP_ONE)), dim3(64), (size_t)pitch * 4, st, a);
    } else if (form == 2) {
        // the dynamic-LDS attribute is per device: one bit per device id (a race here only repeats an idempotent call)
        static std::atomic<unsigned long long> attr_mask{0};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 0;
        if (!((attr_mask.load(std::memory_order_acquire) >> dev) & 1ull)) {
            hipError_t e = hipFuncSetAttribute((const void*)composite_long_kernel<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               CL_LDS_MAX - 2 * CL_LDS_STATIC);
            if (e != hipSuccess) return (int)e;
            attr_mask.fetch_or(1ull << dev, std::memory_order_release);
        }
        hipLaunchKernelGGL((composite_long_kernel<2, 2>), dim3(cl_blocks(n_rays, 2, CL_CAP_TWO)), dim3(128), (size_t)pitch * 8, st, a);
    } else {
        hipLaunchKernelGGL((composite_long_kernel<1, 4>), dim3(cl_blocks(n_rays, 4, CL_CAP_WIDE)), dim3(256), 0, st, a);
    }
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int hav_composite_long_bwd(float* d_rf, const float* d_rgb, const float* d_acc, const float* d_weights, const float* d_depth,
                                      const float* rf, const float* z, const float* rd, const float* noise, const float* bg,
                                      int64_t n_rays, int S, int CH, int n_sigmoid, void* stream)
{
    return hav_composite_long_bwd_form(d_rf, d_rgb, d_acc, d_weights, d_depth, rf, z, rd, noise, bg, n_rays, S, CH, n_sigmoid, 0, stream);
}
