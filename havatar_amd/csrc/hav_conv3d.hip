// hav_conv3d.hip -- the 3x3x3 / stride 1 / zero padding 1 convolutions of the skinning-volume decoder (reference
// model/network/voxel_encoder.py:183-210: UpConv3DBlock = trilinear x2 -> Conv3d(3, padding 1) -> InstanceNorm3d -> ReLU) on the fp16
// matrix cores with split operands, forward, data gradient and weight gradient.  NCDHW fp32 in and out, no layout transposes.
//
//   y[b,o,z,y,x] = bias[o] + sum_{i,kz,ky,kx} w[o,i,kz,ky,kx] * x[b,i,z+kz-1,y+ky-1,x+kx-1]
//
// Same arithmetic as hav_conv.hip: x = xh + xl, w = wh + wl in fp16, three products (wl.xh + wh.xl + wh.xh) on
// v_mfma_f32_32x32x16_f16, fp32 accumulation; both activations and gradients take hav_absmax words and are scaled by a power of two
// into [512, 1024) before the split (exact; undone on the way out).  No float atomics anywhere: K-split slices are added in slice order
// by a second kernel.
//
// Forward / data gradient (conv3d_k3_kernel).  GEMM view: M = Cout (one or two 32-row MFMA tiles per workgroup -- Cout = 16 runs half a
// tile of zero rows, Cout = 128 takes two workgroups per voxel tile), N = voxels, K = 27 Cin.  Workgroup = 4 waves =
// every output channel x a [4 z x 4 y x 16 x] voxel tile; wave w owns
// plane z0 + w, two 32-voxel column blocks (2 rows x 16 columns each).  K runs over 16-channel chunks: the chunk's input patch with its
// halo (6 x 6 x 18 voxels, already split into hi / lo: 80-byte records as in hav_conv.hip) is staged in LDS once and serves all 27 taps
// -- a tap is a record offset.  The weights are pre-split, pre-scaled by their own power of two and arranged per (chunk, tap, M tile, part) by
// hav_conv3d_k3_pack / _pack_t and stream from L2.  The patch is single-buffered (51.8 KB, two barriers per chunk): hiding the staging is left to
// the other workgroups of the CU -- by the compiler's register counts two (Cout >= 64: 184 VGPRs) or three (152) fit; how much they overlap
// has not been measured.  Volumes with too few tiles to fill the GPU split the chunk range over 2-8 workgroups (conv3d_k3_finish_kernel).
// D and H are free (border tiles are masked); W % 16 == 0.
//
// Weight gradient (conv3d_k3_wgrad_kernel): see its header below.
#include "hav_common.h"

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef float fl2_t __attribute__((ext_vector_type(2)));

#define C3_TD 4
#define C3_TH 4
#define C3_TW 16
#define C3_PD (C3_TD + 2)
#define C3_PH (C3_TH + 2)
#define C3_PW (C3_TW + 2)
#define C3_VOX (C3_PD * C3_PH * C3_PW)       // 648 voxels of the staged patch
#define C3_REC 20                            // dwords per voxel record: 8 (hi, 16 ch) + 8 (lo) + 4 pad = 80 bytes
#define C3_TASKS (C3_VOX * 8)                // (voxel, channel pair) staging tasks per chunk
#define C3_TPT ((C3_TASKS + 255) / 256)      // 21 per thread

// e with 2^e * max |x| in [512, 1024) from hav_absmax's words (the rule of hav_conv.hip's amax_pow2)
__device__ __forceinline__ int c3_amax_pow2(const unsigned int* words, int lane, float extra = 1.0f)
{
    static_assert(HAV_ABSMAX_WORDS == 256, "four partial maxima per lane");
    const uint4 w4 = reinterpret_cast<const uint4*>(words)[lane];
    unsigned int mb = w4.x > w4.y ? w4.x : w4.y;
    mb = w4.z > mb ? w4.z : mb;
    mb = w4.w > mb ? w4.w : mb;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const unsigned int t = (unsigned int)__shfl_xor((int)mb, o, 64); mb = t > mb ? t : mb; }
    mb = __float_as_uint(__uint_as_float(mb) * extra);
    const int be = (int)((mb >> 23) & 0xFFu);
    if (be < 1 || be > 254) return 0;
    const int e = 9 - (be - 127);
    return e > 100 ? 100 : (e < -100 ? -100 : e);
}
__device__ __forceinline__ float c3_pow2f(int e) { return __uint_as_float((unsigned int)(127 + e) << 23); }
__device__ __forceinline__ void c3_split2(float v0, float v1, uint32_t& hi, uint32_t& lo)
{
    const fl2_t f = {v0, v1};
    const h2_t hh = __builtin_convertvector(f, h2_t);
    const h2_t ll = __builtin_convertvector(f - __builtin_convertvector(hh, fl2_t), h2_t);
    hi = __builtin_bit_cast(uint32_t, hh); lo = __builtin_bit_cast(uint32_t, ll);
}

static bool c3_channels_ok(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }
static bool c3_shape_ok(int Cin, int Cout, int W) { return c3_channels_ok(Cin) && c3_channels_ok(Cout) && W >= 16 && (W % 16) == 0; }
static int c3_mtiles(int Cout) { return (Cout + 31) / 32; }

// blob = the fragments, then a trailer: HAV_ABSMAX_WORDS words of hav_absmax(w) and the exponent e_w the pack derived from them (the
// weights are stored as w * wmul * 2^e_w, max in [512, 1024): the decoder's filters are initialised at 1e-3 and below, where a fixed
// scale would leave the low parts of the split in the fp16 subnormals; the convolution undoes 2^e_w on the way out)
static int64_t c3_frag_bytes(int Cout, int Cin) { return (int64_t)(Cin / 16) * 27 * c3_mtiles(Cout) * 2 * 64 * 16; }
#define C3_TRAILER_BYTES (HAV_ABSMAX_WORDS * 4 + 16)
extern "C" int64_t hav_conv3d_k3_packed_bytes(int Cout, int Cin)
{
    if (!c3_channels_ok(Cout) || !c3_channels_ok(Cin)) return 0;          // what the packs refuse has no size
    return c3_frag_bytes(Cout, Cin) + C3_TRAILER_BYTES;
}

// fragment (chunk cc, tap t, M tile m, part): lane (i, h) holds W[32m + i][16cc + 8h + e][t] * wmul * 2^e_w, e = 0..7, as fp16 hi or lo;
// rows past Cout are zeros.  transposed: the filters of the data gradient, W'[i][o][t] = w[o][i][26 - t] (Cout, Cin are those of W'),
// read straight from w [Cin, Cout, 27].
__global__ void __launch_bounds__(256) conv3d_k3_pack_kernel(uint4* __restrict__ blob, unsigned int* __restrict__ trailer, const float* __restrict__ w,
                                                             int Cout, int Cin, float wmul, int transposed)
{
    const int cc = blockIdx.x, m = blockIdx.y, MT = gridDim.y, tid = threadIdx.x;
    const int ew = c3_amax_pow2(trailer, tid & 63, fabsf(wmul));
    const float wsc = c3_pow2f(ew);
    if (cc == 0 && m == 0 && tid == 0) trailer[HAV_ABSMAX_WORDS] = (unsigned int)ew;
    for (int q = tid; q < 27 * 2 * 64; q += 256) {
        const int lane = q & 63, part = (q >> 6) & 1, t = q >> 7, i = lane & 31, h = lane >> 5;
        const int o = 32 * m + i;
        uint32_t out[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            float v[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ci = 16 * cc + 8 * h + 2 * d + u;
                float f = 0.f;
                if (o < Cout) f = transposed ? w[((int64_t)ci * Cout + o) * 27 + (26 - t)] : w[((int64_t)o * Cin + ci) * 27 + t];
                v[u] = (f * wmul) * wsc;
            }
            uint32_t hi, lo;
            c3_split2(v[0], v[1], hi, lo);
            out[d] = part ? lo : hi;
        }
        blob[((((int64_t)cc * 27 + t) * MT + m) * 2 + part) * 64 + lane] = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

extern "C" int hav_conv3d_k3_pack(void* blob, const float* w, int Cout, int Cin, float wmul, void* stream)
{
    if (!blob || !w || Cout < 1 || Cin < 1) return HAV_EINVAL;
    if (!c3_channels_ok(Cin) || !c3_channels_ok(Cout)) return HAV_EUNSUP;
    unsigned int* trailer = (unsigned int*)((char*)blob + c3_frag_bytes(Cout, Cin));
    const int rc = hav_absmax(trailer, w, (int64_t)Cout * Cin * 27, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(conv3d_k3_pack_kernel, dim3((unsigned)(Cin / 16), (unsigned)c3_mtiles(Cout)), dim3(256), 0, (hipStream_t)stream, (uint4*)blob, trailer,
                       w, Cout, Cin, wmul, 0);
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int hav_conv3d_k3_pack_t(void* blob, const float* w, int Cout_w, int Cin_w, float wmul, void* stream)
{
    // w [Cout_w, Cin_w, 27] -> the blob of the convolution with Cin_w output and Cout_w input channels (flipped taps)
    if (!blob || !w || Cout_w < 1 || Cin_w < 1) return HAV_EINVAL;
    if (!c3_channels_ok(Cin_w) || !c3_channels_ok(Cout_w)) return HAV_EUNSUP;
    unsigned int* trailer = (unsigned int*)((char*)blob + c3_frag_bytes(Cin_w, Cout_w));
    const int rc = hav_absmax(trailer, w, (int64_t)Cout_w * Cin_w * 27, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(conv3d_k3_pack_kernel, dim3((unsigned)(Cout_w / 16), (unsigned)c3_mtiles(Cin_w)), dim3(256), 0, (hipStream_t)stream, (uint4*)blob, trailer,
                       w, Cin_w, Cout_w, wmul, 1);
    HAV_LAUNCH_CHECK();
    return 0;
}

struct Conv3dArgs {
    float* y; const float* x; const uint4* blob;
    float* partial;          // K-split: [ksplit][B,Cout,D,H,W] sums of the slices (already scaled back), added up by conv3d_k3_finish_kernel
    const unsigned int* in_amax;
    const int* w_exp;          // e_w of the blob's trailer
    const float* bias;
    int ksplit, mgroups, B, Cin, Cout, D, H, W, tz, ty, tx;
};

template <int MT>
__global__ void __launch_bounds__(256, 2) conv3d_k3_kernel(Conv3dArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[C3_VOX * C3_REC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int D = a.D, H = a.H, W = a.W, Cin = a.Cin, NCT = Cin / 16;
    int t = blockIdx.x;
    const int px = t % a.tx; t /= a.tx;
    const int py = t % a.ty; t /= a.ty;
    const int pz = t;
    const int x0 = px * C3_TW, y0 = py * C3_TH, z0 = pz * C3_TD;
    const int b = blockIdx.y, ks = blockIdx.z / a.mgroups, mg = blockIdx.z - ks * a.mgroups;          // mg: 64 output channels
    const int MTT = MT * a.mgroups, m0 = MT * mg;
    const int c_lo = (NCT * ks) / a.ksplit, c_hi = (NCT * (ks + 1)) / a.ksplit;
    const int64_t DHW = (int64_t)D * H * W;
    const float* xb = a.x + (int64_t)b * Cin * DHW;
    float in_sc = 1.0f, out_sc = 1.0f;
    if (a.in_amax) {
        const int e = c3_amax_pow2(a.in_amax, lane);
        in_sc = c3_pow2f(e);
        out_sc = c3_pow2f(-e);
    }
    const float out_w = c3_pow2f(-*a.w_exp);          // applied one after the other: the exponents' sum may pass 127
    // staging tasks of this thread: (channel pair, voxel of the patch) -> one hi dword + one lo dword.  t_off < 0: outside the volume
    // (zeros); t_lds < 0: no task
    int t_off[C3_TPT], t_lds[C3_TPT];
#pragma unroll
    for (int q = 0; q < C3_TPT; ++q) {
        const int task = tid + 256 * q;
        const int cp = task / C3_VOX, p = task - cp * C3_VOX;
        const int vz = p / (C3_PH * C3_PW), r = p - vz * (C3_PH * C3_PW);
        const int vy = r / C3_PW, vx = r - vy * C3_PW;
        const int gz = z0 + vz - 1, gy = y0 + vy - 1, gx = x0 + vx - 1;
        const bool ok = task < C3_TASKS && gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W;
        t_off[q] = ok ? (int)((2 * cp) * DHW + ((int64_t)gz * H + gy) * W + gx) : -1;          // < 2^31: checked by the launcher
        t_lds[q] = task < C3_TASKS ? p * C3_REC + cp : -1;
    }
    f32x16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[m][0][r] = 0.f; acc[m][1][r] = 0.f; }

    for (int cc = c_lo; cc < c_hi; ++cc) {
        const float* src = xb + (int64_t)(16 * cc) * DHW;
        float v[C3_TPT][2];
#pragma unroll
        for (int q = 0; q < C3_TPT; ++q) {
            v[q][0] = t_off[q] >= 0 ? src[t_off[q]] : 0.f;
            v[q][1] = t_off[q] >= 0 ? src[t_off[q] + DHW] : 0.f;
        }
        __syncthreads();          // the previous chunk's reads of the patch are done
#pragma unroll
        for (int q = 0; q < C3_TPT; ++q) {
            if (t_lds[q] < 0) continue;
            uint32_t hi, lo;
            c3_split2(v[q][0] * in_sc, v[q][1] * in_sc, hi, lo);
            lds[t_lds[q]] = hi;
            lds[t_lds[q] + 8] = lo;
        }
        __syncthreads();
        const uint4* ab = a.blob + ((int64_t)(cc * 27) * MTT + m0) * 128 + lane;
#pragma unroll 3
        for (int tap = 0; tap < 27; ++tap) {
            const int kz = tap / 9, ky = (tap - 9 * kz) / 3, kx = tap - 9 * kz - 3 * ky;
            uint4 A[MT][2];
#pragma unroll
            for (int m = 0; m < MT; ++m) { A[m][0] = ab[(int64_t)(tap * MTT + m) * 128]; A[m][1] = ab[(int64_t)(tap * MTT + m) * 128 + 64]; }
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int p = ((wave + kz) * C3_PH + 2 * rr + (j >> 4) + ky) * C3_PW + (j & 15) + kx;
                const uint4 bh = *reinterpret_cast<const uint4*>(lds + p * C3_REC + 4 * h);
                const uint4 bl = *reinterpret_cast<const uint4*>(lds + p * C3_REC + 8 + 4 * h);
                const f16x8_t xh = __builtin_bit_cast(f16x8_t, bh), xl = __builtin_bit_cast(f16x8_t, bl);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const f16x8_t ah = __builtin_bit_cast(f16x8_t, A[m][0]), al = __builtin_bit_cast(f16x8_t, A[m][1]);
                    acc[m][rr] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, xh, acc[m][rr], 0, 0, 0);
                    acc[m][rr] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, xl, acc[m][rr], 0, 0, 0);
                    acc[m][rr] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, xh, acc[m][rr], 0, 0, 0);
                }
            }
        }
    }
    // D[m = o][n = voxel]: lane j = voxel (row j >> 4, column j & 15), registers = o rows
    const int gz = z0 + wave;
    if (gz >= D) return;
    float* dst = a.partial ? a.partial + (int64_t)ks * a.B * a.Cout * DHW : a.y;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int gy = y0 + 2 * rr + (j >> 4), gx = x0 + (j & 15);
        if (gy >= H) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = 32 * (m0 + m) + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co < a.Cout) {
                    float val = acc[m][rr][r] * out_sc * out_w;
                    if (!a.partial && a.bias) val += a.bias[co];
                    dst[((int64_t)b * a.Cout + co) * DHW + ((int64_t)gz * H + gy) * W + gx] = val;
                }
            }
    }
}

// K-split epilogue: y = (sum of the slices, in slice order) + bias
__global__ void __launch_bounds__(256) conv3d_k3_finish_kernel(Conv3dArgs a, int64_t total, int64_t DHW)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int k = 0; k < a.ksplit; ++k) v += a.partial[(int64_t)k * total + e];
        if (a.bias) v += a.bias[(e / DHW) % a.Cout];
        a.y[e] = v;
    }
}

static int64_t c3_tiles(int B, int D, int H, int W) { return (int64_t)B * ((D + C3_TD - 1) / C3_TD) * ((H + C3_TH - 1) / C3_TH) * (W / C3_TW); }
static int c3_ksplit(int B, int Cin, int D, int H, int W)
{
    const int64_t tiles = c3_tiles(B, D, H, W);
    int ks = 1;
    while (tiles * ks < hav_num_cus() && ks < 8 && (Cin / 16) / (ks * 2) >= 1) ks *= 2;
    return ks;
}
static bool c3_size_ok(int B, int Cin, int Cout, int D, int H, int W)
{
    // the kernels index one sample with 32-bit offsets; the grid's y / z dimensions are 16-bit
    const int64_t DHW = (int64_t)D * H * W, big = Cin > Cout ? Cin : Cout;
    return big * DHW < ((int64_t)1 << 31) && B <= 65535;
}

extern "C" int64_t hav_conv3d_k3_scratch_bytes(int B, int Cin, int Cout, int D, int H, int W)
{
    if (B < 1 || D < 1 || H < 1 || !c3_shape_ok(Cin, Cout, W) || !c3_size_ok(B, Cin, Cout, D, H, W)) return 0;
    const int ks = c3_ksplit(B, Cin, D, H, W);
    return ks > 1 ? (int64_t)ks * B * Cout * D * H * W * 4 : 0;
}

extern "C" int hav_conv3d_k3_fwd(float* y, const float* x, const void* packed, const float* bias, const void* in_amax, int B, int Cin, int Cout,
                                 int D, int H, int W, void* scratch, void* stream)
{
    if (!y || !x || !packed || B < 1 || Cin < 1 || Cout < 1 || D < 1 || H < 1 || W < 1) return HAV_EINVAL;
    if (!c3_shape_ok(Cin, Cout, W) || !c3_size_ok(B, Cin, Cout, D, H, W)) return HAV_EUNSUP;
    Conv3dArgs a;
    a.w_exp = (const int*)((const char*)packed + c3_frag_bytes(Cout, Cin) + HAV_ABSMAX_WORDS * 4);
    a.y = y; a.x = x; a.blob = (const uint4*)packed; a.in_amax = (const unsigned int*)in_amax; a.bias = bias;
    a.ksplit = scratch ? c3_ksplit(B, Cin, D, H, W) : 1;
    a.partial = a.ksplit > 1 ? (float*)scratch : nullptr;
    a.B = B; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
    a.tz = (D + C3_TD - 1) / C3_TD; a.ty = (H + C3_TH - 1) / C3_TH; a.tx = W / C3_TW;
    const int64_t tiles = (int64_t)a.tz * a.ty * a.tx;
    if (tiles > 0x7fffffff) return HAV_EUNSUP;
    a.mgroups = Cout > 64 ? Cout / 64 : 1;
    const dim3 grid((unsigned)tiles, (unsigned)B, (unsigned)(a.ksplit * a.mgroups));
    if (Cout >= 64) hipLaunchKernelGGL(conv3d_k3_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(conv3d_k3_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
    HAV_LAUNCH_CHECK();
    if (a.partial) {
        const int64_t DHW = (int64_t)D * H * W, total = (int64_t)B * Cout * DHW;
        hipLaunchKernelGGL(conv3d_k3_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, total, DHW);
        HAV_LAUNCH_CHECK();
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Weight gradient:  gw[o, i, kz, ky, kx] = sum_{b, z, y, x} g[b, o, z, y, x] * xin[b, i, z + kz - 1, y + ky - 1, x + kx - 1]
//
// GEMM view as in conv3x3_wgrad_kernel (hav_conv.hip): M = Cout, N = Cin, K = voxels, per tap a different shift of the N operand; both
// operands are activations and go through LDS as fp16 hi / lo, each with its own power of two.  Workgroup = 32 (o) x 32 (i) x 27 taps
// (channel counts of 16 run half a tile of zeros); wave w owns taps 7 w .. 7 w + 6 (the last one six).  A work unit is a column strip
// (b, INPUT plane zi, 16 columns x0, up to 16 rows): K advances one 16-voxel row segment per step down the strip; the step at row y
// needs input rows y - 1, y, y + 1 of plane zi (a ring of four LDS slots, each row stored three times, shifted by kx - 1 voxels: an
// MFMA operand is 8 consecutive fp16) and row y of g in the three planes zi + 1 - kz that plane zi feeds -- so a step stages ONE new
// input row and three g rows, and the three planes of x never sit in LDS together.  Units are dealt to gridDim.z workgroups per output
// block, at most one per compute unit; a workgroup walks its units in a fixed order.  Partial sums are [z][tap][o][i]; the bias
// gradient's partial sums are [o][64 slices].  conv3d_k3_wgrad_reduce_kernel adds both up in a fixed order.
#define W3_XI 52            // dwords per input channel in a row slot: 3 shifts x 16 (8 hi + 8 lo) + 4 pad
#define W3_GO 20            // dwords per output channel in a g buffer: 8 hi + 8 lo + 4 pad
#define W3_SEG 16           // rows per work unit
#define W3_BSL 64           // slices of the bias gradient's first pass
struct Wgrad3dArgs {
    float* partial; const float* g; const float* x; const unsigned int* g_amax; const unsigned int* x_amax;
    int B, Cin, Cout, D, H, W, units, segs;
};

__global__ void __launch_bounds__(256, 2) conv3d_k3_wgrad_kernel(Wgrad3dArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t xs[4][32 * W3_XI];
    __shared__ __attribute__((aligned(16))) uint32_t gs[2][3][32 * W3_GO];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
    const int D = a.D, H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
    const int64_t HW = (int64_t)H * W, DHW = (int64_t)D * HW;
    const int sw = W / 16;
    const int eg = a.g_amax ? c3_amax_pow2(a.g_amax, lane) : 0;
    const int ex = a.x_amax ? c3_amax_pow2(a.x_amax, lane) : 0;
    const float g_sc = c3_pow2f(eg), x_sc = c3_pow2f(ex);
    const float out_g = c3_pow2f(-eg), out_x = c3_pow2f(-ex);          // applied one after the other: |eg + ex| may pass 127
    // staging roles.  x: thread = (i = tid >> 3, voxel pair tid & 7).  g: thread = (o = (tid >> 2) & 31, 4 voxels tid & 3) for planes
    // kz = tid >> 7 and, threads 0-127 only, kz = 2
    const int x_i = tid >> 3, x_p = tid & 7;
    const int g_o = (tid >> 2) & 31, g_q = tid & 3, g_k = tid >> 7;
    const bool x_ch = i0 + x_i < Cin, g_ch = o0 + g_o < Cout;
    f32x16 acc[7];
#pragma unroll
    for (int t = 0; t < 7; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    struct XR { float a0, a1, el, er; };
    auto fetch_x = [&](int b, int zi, int x0, int row) {
        XR r = {0.f, 0.f, 0.f, 0.f};
        if (x_ch && row >= 0 && row < H) {
            const float* src = a.x + ((int64_t)b * Cin + i0 + x_i) * DHW + (int64_t)zi * HW + (int64_t)row * W + x0;
            const float2 v = *reinterpret_cast<const float2*>(src + 2 * x_p);
            r.a0 = v.x; r.a1 = v.y;
            if (x_p == 0 && x0 > 0) r.el = src[-1];
            if (x_p == 7 && x0 + 16 < W) r.er = src[16];
        }
        return r;
    };
    auto stash_x = [&](int row, const XR& r) {
        uint32_t* dst = xs[(row + 1) & 3] + x_i * W3_XI;
        float pa1 = __shfl_up(r.a1, 1, 64), na0 = __shfl_down(r.a0, 1, 64);
        if (x_p == 0) pa1 = r.el;
        if (x_p == 7) na0 = r.er;
        const float a0 = r.a0 * x_sc, a1 = r.a1 * x_sc;
        pa1 *= x_sc; na0 *= x_sc;
        uint32_t hi, lo;
        c3_split2(pa1, a0, hi, lo); dst[0 * 16 + x_p] = hi; dst[0 * 16 + 8 + x_p] = lo;          // kx = 0: element e = x[x0 + e - 1]
        c3_split2(a0, a1, hi, lo);  dst[1 * 16 + x_p] = hi; dst[1 * 16 + 8 + x_p] = lo;          // kx = 1
        c3_split2(a1, na0, hi, lo); dst[2 * 16 + x_p] = hi; dst[2 * 16 + 8 + x_p] = lo;          // kx = 2: element e = x[x0 + e + 1]
    };
    // g row `row` of plane zi + 1 - kz (zeros outside the volume)
    auto fetch_g = [&](int b, int zi, int x0, int row, int kz) {
        const int zo = zi + 1 - kz;
        if (!g_ch || zo < 0 || zo >= D) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4*>(a.g + ((int64_t)b * Cout + o0 + g_o) * DHW + (int64_t)zo * HW + (int64_t)row * W + x0 + 4 * g_q);
    };
    auto stash_g = [&](int buf, int kz, const float4& v) {
        uint32_t* dst = gs[buf][kz] + g_o * W3_GO + 2 * g_q;
        uint32_t h0, l0, h1, l1;
        c3_split2(v.x * g_sc, v.y * g_sc, h0, l0);
        c3_split2(v.z * g_sc, v.w * g_sc, h1, l1);
        dst[0] = h0; dst[1] = h1; dst[8] = l0; dst[9] = l1;
    };

    for (int s = blockIdx.z; s < a.units; s += gridDim.z) {
        int u = s;
        const int seg = u % a.segs; u /= a.segs;
        const int x0 = (u % sw) * 16; u /= sw;
        const int zi = u % D, b = u / D;
        const int ya = seg * W3_SEG, yb = ya + W3_SEG < H ? ya + W3_SEG : H;
        __syncthreads();          // the previous unit's last step is done with the ring
        stash_x(ya - 1, fetch_x(b, zi, x0, ya - 1));
        stash_x(ya, fetch_x(b, zi, x0, ya));
        stash_x(ya + 1, fetch_x(b, zi, x0, ya + 1));
        stash_g(ya & 1, g_k, fetch_g(b, zi, x0, ya, g_k));
        if (tid < 128) stash_g(ya & 1, 2, fetch_g(b, zi, x0, ya, 2));
        __syncthreads();
        for (int y = ya; y < yb; ++y) {
            // next step's operands: input row y + 2 (its slot held row y - 2) and g rows y + 1 (other buffer): loads now, LDS after the MFMAs
            const bool more = y + 1 < yb;
            XR nx = {0.f, 0.f, 0.f, 0.f};
            float4 ng0 = make_float4(0.f, 0.f, 0.f, 0.f), ng1 = ng0;
            if (more) {
                nx = fetch_x(b, zi, x0, y + 2);
                ng0 = fetch_g(b, zi, x0, y + 1, g_k);
                if (tid < 128) ng1 = fetch_g(b, zi, x0, y + 1, 2);
            }
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const int t = wave * 7 + q;          // tap (wave-uniform); wave 3 has six (t = 21..26)
                if (t < 27) {
                    const int kz = t / 9, ky = (t - 9 * kz) / 3, kx = t - 9 * kz - 3 * ky;
                    const uint32_t* G = gs[y & 1][kz] + j * W3_GO + 4 * h;
                    const f16x8_t gh = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(G));
                    const f16x8_t gl = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(G + 8));
                    const uint32_t* X = xs[(y + ky) & 3] + j * W3_XI + kx * 16 + 4 * h;          // row y + ky - 1 -> slot (y + ky) & 3
                    const f16x8_t xh = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(X));
                    const f16x8_t xl = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(X + 8));
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl, xh, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, xl, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, xh, acc[q], 0, 0, 0);
                }
            }
            if (more) {
                stash_x(y + 2, nx);
                stash_g((y + 1) & 1, g_k, ng0);
                if (tid < 128) stash_g((y + 1) & 1, 2, ng1);
            }
            __syncthreads();
        }
    }
    // D[m = o][n = i]: lane j = i, registers = o rows.  partial[z][t][o][i]
    float* pp = a.partial + (int64_t)blockIdx.z * 27 * Cout * Cin;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const int t = wave * 7 + q;
        if (t < 27 && i0 + j < Cin) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (o < Cout) pp[((int64_t)t * Cout + o) * Cin + i0 + j] = acc[q][r] * out_g * out_x;
            }
        }
    }
}

// first pass of the bias gradient: block (slice, o) sums its slice of g[:, o] (fixed order inside the block)
__global__ void __launch_bounds__(256) conv3d_k3_gbias_kernel(float* __restrict__ part, const float* __restrict__ g, int B, int Cout, int64_t DHW)
{
    __shared__ float red[256];
    const int sl = blockIdx.x, o = blockIdx.y;
    const int64_t n4 = DHW >> 2, per = (n4 + W3_BSL - 1) / W3_BSL;          // DHW % 16 == 0
    const int64_t lo = per * sl, hi = lo + per < n4 ? lo + per : n4;
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        const float4* g4 = reinterpret_cast<const float4*>(g + ((int64_t)b * Cout + o) * DHW);
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) { const float4 v = g4[i]; s += (v.x + v.y) + (v.z + v.w); }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[o * W3_BSL + sl] = red[0];
}

__global__ void __launch_bounds__(256) conv3d_k3_wgrad_reduce_kernel(float* __restrict__ gw, float* __restrict__ gbias, const float* __restrict__ partial,
                                                                     const float* __restrict__ bpart, int ks, int Cout, int Cin)
{
    const int64_t n = (int64_t)Cout * Cin, wn = gw ? n * 27 : 0, total = wn + (gbias ? Cout : 0);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        if (e < wn) {
            const int64_t oi = e / 27, t = e - oi * 27;
            for (int k = 0; k < ks; ++k) s += partial[((int64_t)k * 27 + t) * n + oi];
            gw[e] = s;
        } else {
            const int o = (int)(e - wn);
            for (int k = 0; k < W3_BSL; ++k) s += bpart[o * W3_BSL + k];
            gbias[o] = s;
        }
    }
}

static int w3_units(int B, int D, int H, int W) { return B * D * (W / 16) * ((H + W3_SEG - 1) / W3_SEG); }
static int w3_ksplit(int B, int Cin, int Cout, int D, int H, int W)
{
    const int blocks = ((Cin + 31) / 32) * ((Cout + 31) / 32), units = w3_units(B, D, H, W);
    int ks = (hav_num_cus() + blocks - 1) / blocks;
    if (ks > units) ks = units;
    return ks < 1 ? 1 : ks;
}
static bool w3_ok(int B, int Cin, int Cout, int D, int H, int W)
{
    return c3_shape_ok(Cin, Cout, W) && c3_size_ok(B, Cin, Cout, D, H, W) && (int64_t)B * D * (W / 16) * ((H + W3_SEG - 1) / W3_SEG) < ((int64_t)1 << 30);
}
extern "C" int64_t hav_conv3d_k3_wgrad_scratch_bytes(int B, int Cin, int Cout, int D, int H, int W)
{
    if (B < 1 || D < 1 || H < 1 || !w3_ok(B, Cin, Cout, D, H, W)) return 0;
    return ((int64_t)w3_ksplit(B, Cin, Cout, D, H, W) * 27 * Cout * Cin + (int64_t)Cout * W3_BSL) * 4;
}

extern "C" int hav_conv3d_k3_wgrad(float* gw, float* gbias, const float* g, const float* x, void* scratch, const void* g_amax, const void* x_amax,
                                   int B, int Cin, int Cout, int D, int H, int W, void* stream)
{
    if ((!gw && !gbias) || !g || !x || !scratch || B < 1 || Cin < 1 || Cout < 1 || D < 1 || H < 1 || W < 1) return HAV_EINVAL;
    if (!w3_ok(B, Cin, Cout, D, H, W)) return HAV_EUNSUP;
    Wgrad3dArgs a;
    a.partial = (float*)scratch; a.g = g; a.x = x; a.g_amax = (const unsigned int*)g_amax; a.x_amax = (const unsigned int*)x_amax;
    a.B = B; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
    a.segs = (H + W3_SEG - 1) / W3_SEG; a.units = w3_units(B, D, H, W);
    const int ks = w3_ksplit(B, Cin, Cout, D, H, W);
    if (gw) {          // NULL: the bias gradient alone
        hipLaunchKernelGGL(conv3d_k3_wgrad_kernel, dim3((unsigned)((Cin + 31) / 32), (unsigned)((Cout + 31) / 32), (unsigned)ks), dim3(256), 0,
                           (hipStream_t)stream, a);
        HAV_LAUNCH_CHECK();
    }
    float* bpart = (float*)scratch + (int64_t)ks * 27 * Cout * Cin;
    if (gbias) {
        hipLaunchKernelGGL(conv3d_k3_gbias_kernel, dim3(W3_BSL, (unsigned)Cout), dim3(256), 0, (hipStream_t)stream, bpart, g, B, Cout, (int64_t)D * H * W);
        HAV_LAUNCH_CHECK();
    }
    const int64_t total = (int64_t)Cout * Cin * 27 + Cout;
    hipLaunchKernelGGL(conv3d_k3_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gw, gbias,
                       (const float*)scratch, (const float*)bpart, ks, Cout, Cin);
    HAV_LAUNCH_CHECK();
    return 0;
}
