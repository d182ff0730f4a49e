// hav_gbuffer.hip -- image-space geometry of a rendered frame, gfx950: metric depth, camera-facing normals and a headlight shade from the maps the
// ray march already produced (depth = sum w z, acc = sum w) and the ray table it read.  The kernel behind havatar_amd.geometry.gbuffer
// (native/gbuffer_ops.py).  No reference counterpart: the reference drops the depth map.
//
// Definition (include/havatar.h states it in full; geometry.gbuffer_statement states it on ATen, tests/test_gbuffer_cpu.py in plain loops).
//   valid = acc > acc_min and isfinite(depth);  z = clamp(depth / acc, near, far) where valid, else 0;  p = o + d z.
//   Tangent along an axis: a side is usable when the neighbour is in the image and both pixels are valid; a+ = |z+ - z|, a- = |z - z-|.
//   Both usable and max(a+, a-) <= 4 min(a+, a-): central, p+ - p-; else the usable side with the smaller a (tie: +); else none.
//   n = tx x ty, negated where n . d > 0; normal = n / |n| where both tangents exist and |n| is finite and positive, else 0.
//
//   gbuffer_kernel   one launch for all B frames; a 256-thread workgroup owns a GB_TH x GB_TW = 4 x 64 pixel tile (a wave = one row of 64
//                    pixels: its loads and stores are row-contiguous).  Every thread evaluates its own pixel (ray row as two float4 at
//                    stride 8) and keeps o, d, near, far, z in registers; threads 0..139 evaluate one pixel of the one-pixel ring around the
//                    tile as well.  p, z and validity of the 6 x 66 pixels go to LDS (struct of arrays: lanes read consecutive banks); after one
//                    barrier each thread forms its two tangents from LDS and writes every output it was given.  An input element is read once,
//                    but for the ring (140 / 256 of a tile more); an output element is written exactly once.
//   Byte outputs     with W a multiple of 4 and dword-aligned pointers, four neighbouring lanes share their bytes by wave shuffles and store
//                    dwords: mask / shade8 / choice one dword per 4 lanes, depth16 one per 2 lanes, normal8 three per 4 lanes.  Any other
//                    width stores bytes.
// The arithmetic is written without contraction (no FMA is formed): the statement on ATen rounds after every operation, and so does this.
// No atomics, no allocation, no synchronisation, no environment reads: the same inputs give the same bits, and the launch can be captured.
// LDS: 4 x 396 floats + 396 bytes = 6732 bytes per workgroup.
#include "hav_common.h"

#include <cmath>

#pragma clang fp contract(off)

#define GB_TH 4
#define GB_TW 64
#define GB_THREADS (GB_TH * GB_TW)
#define GB_HW (GB_TW + 2)                          // halo row
#define GB_HALO ((GB_TH + 2) * GB_HW)              // 396 staged pixels
#define GB_RING (2 * GB_HW + 2 * GB_TH)            // 140 of them lie around the tile

static_assert(GB_TW % 64 == 0 && GB_THREADS == 256 && GB_RING <= GB_THREADS, "a wave owns whole rows; one ring pixel per thread at most");

struct GbOut {
    float* z;
    float* normal;
    uint8_t* mask;
    uint8_t* depth16;
    uint8_t* normal8;
    uint8_t* shade8;
    uint8_t* choice;
};

struct GbPix {
    float ox, oy, oz, dx, dy, dz, nr, fr, z;
    bool valid;
};

__device__ __forceinline__ GbPix gb_pixel(const float* __restrict__ rays, const float* __restrict__ depth, const float* __restrict__ acc, int idx,
                                          int stride, float acc_min, bool vec)
{
    GbPix q;
    const float* r = rays + (int64_t)idx * stride;
    if (vec) {
        const float4 a = reinterpret_cast<const float4*>(r)[0], b = reinterpret_cast<const float4*>(r)[1];
        q.ox = a.x; q.oy = a.y; q.oz = a.z; q.dx = a.w; q.dy = b.x; q.dz = b.y; q.nr = b.z; q.fr = b.w;
    } else {
        q.ox = r[0]; q.oy = r[1]; q.oz = r[2]; q.dx = r[3]; q.dy = r[4]; q.dz = r[5]; q.nr = r[6]; q.fr = r[7];
    }
    const float dep = depth[idx], a = acc[idx];
    q.valid = a > acc_min && std::isfinite(dep);
    float t = dep / a;
    t = t < q.nr ? q.nr : t;
    t = t > q.fr ? q.fr : t;
    q.z = q.valid ? t : 0.f;
    return q;
}

// tangent along one axis of the staged tile: side bit 0 = the + neighbour is used, bit 1 = the - neighbour
__device__ __forceinline__ int gb_tangent(float t[3], const float* sX, const float* sY, const float* sZ, const float* sD, const uint8_t* sV, int c, int s,
                                          float z, bool valid)
{
    const bool vp = valid && sV[c + s], vm = valid && sV[c - s];
    const float ap = fabsf(sD[c + s] - z), am = fabsf(z - sD[c - s]);
    const float mx = ap > am ? ap : am, mn = ap > am ? am : ap;
    const int side = (vp && vm && mx <= 4.f * mn) ? 3 : (vp && (!vm || ap <= am)) ? 1 : vm ? 2 : 0;
    const int hi = (side & 1) ? c + s : c, lo = (side & 2) ? c - s : c;
    t[0] = sX[hi] - sX[lo];
    t[1] = sY[hi] - sY[lo];
    t[2] = sZ[hi] - sZ[lo];
    return side;
}

// the bytes of four neighbouring lanes in one dword: meaningful in lanes 0, 4, 8, ...; every lane of the wave calls it
__device__ __forceinline__ uint32_t gb_pack4(uint32_t v)
{
    const uint32_t a = v | ((uint32_t)__shfl_down(v, 1, 64) << 8);
    return a | ((uint32_t)__shfl_down(a, 2, 64) << 16);
}

__global__ void __launch_bounds__(GB_THREADS) gbuffer_kernel(GbOut out, const float* __restrict__ rays, const float* __restrict__ depth,
                                                             const float* __restrict__ acc, int H, int W, int stride, int tiles_x, int tiles_y,
                                                             float acc_min, int vec, int packed)
{
    __shared__ float sX[GB_HALO], sY[GB_HALO], sZ[GB_HALO], sD[GB_HALO];
    __shared__ uint8_t sV[GB_HALO];
    const int tid = threadIdx.x, lx = tid & (GB_TW - 1), ly = tid / GB_TW;
    const int tile = blockIdx.x, tx = tile % tiles_x, tr = tile / tiles_x, ty = tr % tiles_y, b = tr / tiles_y;
    const int gx = tx * GB_TW + lx, gy = ty * GB_TH + ly;
    const bool live = gx < W && gy < H;
    const int idx = (b * H + gy) * W + gx;          // < B H W where live; not used otherwise
    const int c = (ly + 1) * GB_HW + lx + 1;

    GbPix q = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
    if (live) q = gb_pixel(rays, depth, acc, idx, stride, acc_min, vec != 0);
    sX[c] = q.ox + q.dx * q.z;
    sY[c] = q.oy + q.dy * q.z;
    sZ[c] = q.oz + q.dz * q.z;
    sD[c] = q.z;
    sV[c] = q.valid ? 1 : 0;
    if (tid < GB_RING) {
        int hy, hx;
        if (tid < GB_HW) { hy = 0; hx = tid; }
        else if (tid < 2 * GB_HW) { hy = GB_TH + 1; hx = tid - GB_HW; }
        else if (tid < 2 * GB_HW + GB_TH) { hy = 1 + tid - 2 * GB_HW; hx = 0; }
        else { hy = 1 + tid - 2 * GB_HW - GB_TH; hx = GB_HW - 1; }
        const int ry = ty * GB_TH + hy - 1, rx = tx * GB_TW + hx - 1;
        GbPix n = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
        if (ry >= 0 && ry < H && rx >= 0 && rx < W) n = gb_pixel(rays, depth, acc, (b * H + ry) * W + rx, stride, acc_min, vec != 0);
        const int h = hy * GB_HW + hx;
        sX[h] = n.ox + n.dx * n.z;
        sY[h] = n.oy + n.dy * n.z;
        sZ[h] = n.oz + n.dz * n.z;
        sD[h] = n.z;
        sV[h] = n.valid ? 1 : 0;
    }
    __syncthreads();

    float tx3[3], ty3[3];
    const int sx = gb_tangent(tx3, sX, sY, sZ, sD, sV, c, 1, q.z, q.valid);
    const int sy = gb_tangent(ty3, sX, sY, sZ, sD, sV, c, GB_HW, q.z, q.valid);
    float nx = tx3[1] * ty3[2] - tx3[2] * ty3[1];
    float ny = tx3[2] * ty3[0] - tx3[0] * ty3[2];
    float nz = tx3[0] * ty3[1] - tx3[1] * ty3[0];
    const bool flip = nx * q.dx + ny * q.dy + nz * q.dz > 0.f;
    if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    const bool has = sx != 0 && sy != 0 && std::isfinite(len) && len > 0.f;
    nx = has ? nx / len : 0.f;
    ny = has ? ny / len : 0.f;
    nz = has ? nz / len : 0.f;

    // the codes
    const uint32_t m = (q.valid ? 1u : 0u) | (has ? 2u : 0u);
    const uint32_t ch = (uint32_t)sx | ((uint32_t)sy << 2) | (flip ? 16u : 0u);
    const float dc = rintf((q.z - q.nr) / (q.fr - q.nr) * 65534.f);
    const uint32_t code = !q.valid ? 0u : dc >= 65534.f ? 65535u : dc >= 0.f ? 1u + (uint32_t)dc : 1u;
    const uint32_t d16 = (code >> 8) | ((code & 255u) << 8);          // the high byte first in memory
    uint32_t n24 = 0;
    if (has)
        n24 = (uint32_t)rintf((nx * 0.5f + 0.5f) * 255.f) | ((uint32_t)rintf((ny * 0.5f + 0.5f) * 255.f) << 8)
              | ((uint32_t)rintf((nz * 0.5f + 0.5f) * 255.f) << 16);
    float lam = -(nx * q.dx + ny * q.dy + nz * q.dz);
    lam = lam > 0.f ? lam : 0.f;
    const float sc = rintf(255.f * lam);
    const uint32_t sh = !has ? 255u : sc >= 255.f ? 255u : (uint32_t)sc;

    if (live) {
        if (out.z) out.z[idx] = q.z;
        if (out.normal) {
            out.normal[3 * idx + 0] = nx;
            out.normal[3 * idx + 1] = ny;
            out.normal[3 * idx + 2] = nz;
        }
    }
    if (packed) {          // uniform over the launch: W is a multiple of 4, so the four lanes of a group are live together and idx is one too
        const int j = lx & 3;
        const uint32_t m4 = gb_pack4(m), s4 = gb_pack4(sh), c4 = gb_pack4(ch);
        const uint32_t d2 = d16 | ((uint32_t)__shfl_down(d16, 1, 64) << 16);
        const uint32_t nn = (uint32_t)__shfl_down(n24, 1, 64);
        if (live) {
            if (j == 0) {
                if (out.mask) reinterpret_cast<uint32_t*>(out.mask)[idx >> 2] = m4;
                if (out.shade8) reinterpret_cast<uint32_t*>(out.shade8)[idx >> 2] = s4;
                if (out.choice) reinterpret_cast<uint32_t*>(out.choice)[idx >> 2] = c4;
            }
            if ((j & 1) == 0 && out.depth16) reinterpret_cast<uint32_t*>(out.depth16)[idx >> 1] = d2;
            if (j < 3 && out.normal8) reinterpret_cast<uint32_t*>(out.normal8)[3 * ((idx - j) >> 2) + j] = (n24 >> (8 * j)) | (nn << (24 - 8 * j));
        }
    } else if (live) {
        if (out.mask) out.mask[idx] = (uint8_t)m;
        if (out.shade8) out.shade8[idx] = (uint8_t)sh;
        if (out.choice) out.choice[idx] = (uint8_t)ch;
        if (out.depth16) {
            out.depth16[2 * idx + 0] = (uint8_t)(code >> 8);
            out.depth16[2 * idx + 1] = (uint8_t)(code & 255u);
        }
        if (out.normal8) {
            out.normal8[3 * idx + 0] = (uint8_t)(n24 & 255u);
            out.normal8[3 * idx + 1] = (uint8_t)((n24 >> 8) & 255u);
            out.normal8[3 * idx + 2] = (uint8_t)(n24 >> 16);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
extern "C" int hav_gbuffer_tile(int axis) { return axis == 0 ? GB_TH : axis == 1 ? GB_TW : 0; }

extern "C" int hav_gbuffer_f32(float* z, float* normal, uint8_t* mask, uint8_t* depth16, uint8_t* normal8, uint8_t* shade8, uint8_t* choice,
                               const float* rays, const float* depth, const float* acc, int B, int H, int W, int stride, float acc_min,
                               void* stream_)
{
    if (!rays || !depth || !acc || B < 1 || H < 1 || W < 1 || stride < 8 || !std::isfinite(acc_min)) return HAV_EINVAL;
    if (!z && !normal && !mask && !depth16 && !normal8 && !shade8 && !choice) return HAV_EINVAL;
    if ((int64_t)B * H * W * stride >= (1LL << 31)) return HAV_EINVAL;
    const int tiles_x = (W + GB_TW - 1) / GB_TW, tiles_y = (H + GB_TH - 1) / GB_TH;
    const int64_t tiles = (int64_t)B * tiles_x * tiles_y;          // < 2^28 + B (tiles_x + tiles_y): a grid dimension holds it
    const int vec = stride == 8 && ((uintptr_t)rays & 15) == 0;
    const uintptr_t bytes = (uintptr_t)mask | (uintptr_t)depth16 | (uintptr_t)normal8 | (uintptr_t)shade8 | (uintptr_t)choice;
    const int packed = W % 4 == 0 && (bytes & 3) == 0;
    GbOut out = {z, normal, mask, depth16, normal8, shade8, choice};
    hipLaunchKernelGGL(gbuffer_kernel, dim3((unsigned)tiles), dim3(GB_THREADS), 0, (hipStream_t)stream_, out, rays, depth, acc, H, W, stride,
                       tiles_x, tiles_y, acc_min, vec, packed);
    HAV_LAUNCH_CHECK();
    return 0;
}
