// hav_raster.hip -- the three orthographic condition renders of a tracked head mesh, gfx950: z-buffered triangle rasterisation with ambient
// vertex colours, the reference's depth-to-normal pass and the 7-channel condition planes.  The kernels behind
// havatar_amd.conditions.render_conditions (native/raster_ops.py).  The reference renders these offline with pytorch3d
// (data_preprocessing/fit_video.py::render_canonical_ortho); nothing of that is used here.
//
// Definition (include/havatar.h states it in full; conditions.conditions_statement states it on ATen, tests/test_conditions_cpu.py in plain loops).
//
//   raster_setup_kernel    thread n < B 3 V: warps vertex (b, v) and rotates it into view k, screen[b][k][v] = (x, y, z + cam_dist, 0) as one
//                          float4; thread n < B 3 H W: keys[n] = all ones.
//   raster_cover_kernel    one thread per (b, k, triangle).  It reads the three corners, forms the exact pixel box of the closed bounding box
//                          (a conservative guess from the inverse pixel map, tightened against the pixel centres themselves: at most three
//                          steps a side) and, for a box of at most RS_BIG pixels, walks it.  Wider boxes are left to the wave: the lanes'
//                          wide triangles are taken one after the other (ballot), all 64 lanes stride one box, so no single thread ever walks a
//                          full-frame triangle.  A hit issues one 64-bit atomic min of key = bits(z) << 32 | face: z >= 0 makes the float's
//                          bits monotonic, the face index in the low word is the tie rule, and a minimum does not depend on arrival order.
//                          A plain load of the key first drops hits that already lost (a stale value only lets a lost hit through to the atomic).
//   raster_resolve_kernel  one thread per pixel, a 256-thread workgroup per RS_TH x RS_TW = 4 x 64 tile (a wave = one row segment of 64 pixels).
//                          Decodes the winner, recomputes its barycentrics with the code the cover kernel ran, interpolates the colour, reads
//                          the four neighbours' depth from their keys and writes every output it was given, cond directly as [B,3,7,H,W].
// The arithmetic is written without contraction (no FMA is formed): the statement on ATen rounds after every operation, and so does this.
// No allocation, no synchronisation, no environment reads; integer atomics only: the same inputs give the same bits, and the three launches
// can be captured.  No LDS.
#include "hav_common.h"

#include <cmath>

#pragma clang fp contract(off)

#define RS_TH 4
#define RS_TW 64
#define RS_THREADS 256
#define RS_BIG 64          // a box of more pixels than this is walked by a wave
#define RS_EMPTY 0xFFFFFFFFFFFFFFFFull

static_assert(RS_TH * RS_TW == RS_THREADS && RS_TW % 64 == 0 && RS_THREADS % 64 == 0, "a wave owns one row segment; whole waves");

struct RsView {
    float scale[3], trans[3], rot[3][3][3], cam_dist;
};

struct RsTri {
    float ax, ay, az, bx, by, bz, cx, cy, cz, area;
    int j0, j1, i0, i1;          // the exact pixel box; empty (j0 > j1 or i0 > i1) for a triangle that takes no part
};

__device__ __forceinline__ float rs_centre(int j, float n) { return (float)(2 * j + 1) / n - 1.f; }

// pixels whose centre lies in [lo, hi]: a guess one pixel wide of the inverse map, moved inwards until the centres themselves agree
__device__ __forceinline__ void rs_span(float lo, float hi, int n, int& p0, int& p1)
{
    const float fn = (float)n;
    float a = (lo + 1.f) * 0.5f * fn - 0.5f, b = (hi + 1.f) * 0.5f * fn - 0.5f;
    a = a < -1.f ? -1.f : (a > fn ? fn : a);          // finite inputs; clamped before the conversion to int
    b = b < -1.f ? -1.f : (b > fn ? fn : b);
    p0 = (int)floorf(a) - 1;
    p1 = (int)ceilf(b) + 1;
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > n - 1 ? n - 1 : p1;
    while (p0 <= p1 && rs_centre(p0, fn) < lo) ++p0;
    while (p1 >= p0 && rs_centre(p1, fn) > hi) --p1;
}

__device__ __forceinline__ void rs_corners(RsTri& t, const float4* __restrict__ scr, int ia, int ib, int ic)
{
    const float4 a = scr[ia], b = scr[ib], c = scr[ic];
    t.ax = a.x; t.ay = a.y; t.az = a.z;
    t.bx = b.x; t.by = b.y; t.bz = b.z;
    t.cx = c.x; t.cy = c.y; t.cz = c.z;
    t.area = (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax);
}

// triangle f of view-batch bv: corners, area and pixel box
__device__ __forceinline__ RsTri rs_triangle(const float4* __restrict__ screen, const int32_t* __restrict__ tris, int64_t bv, int f, int V, int H, int W)
{
    RsTri t;
    t.j0 = t.i0 = 0;
    t.j1 = t.i1 = -1;
    const int ia = tris[3 * (int64_t)f + 0], ib = tris[3 * (int64_t)f + 1], ic = tris[3 * (int64_t)f + 2];
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) return t;
    rs_corners(t, screen + bv * V, ia, ib, ic);
    const bool finite = std::isfinite(t.ax) && std::isfinite(t.ay) && std::isfinite(t.az) && std::isfinite(t.bx) && std::isfinite(t.by)
                        && std::isfinite(t.bz) && std::isfinite(t.cx) && std::isfinite(t.cy) && std::isfinite(t.cz);
    if (!finite || t.area == 0.f) return t;
    const float lox = fminf(fminf(t.ax, t.bx), t.cx), hix = fmaxf(fmaxf(t.ax, t.bx), t.cx);
    const float loy = fminf(fminf(t.ay, t.by), t.cy), hiy = fmaxf(fmaxf(t.ay, t.by), t.cy);
    rs_span(lox, hix, W, t.j0, t.j1);
    rs_span(loy, hiy, H, t.i0, t.i1);
    return t;
}

// step 5 at one pixel centre inside the triangle's box
__device__ __forceinline__ bool rs_hit(const RsTri& t, float X, float Y, float& z, float& b0, float& b1, float& b2)
{
    const float w0 = (t.bx - X) * (t.cy - Y) - (t.by - Y) * (t.cx - X);
    const float w1 = (t.cx - X) * (t.ay - Y) - (t.cy - Y) * (t.ax - X);
    const float w2 = (t.ax - X) * (t.by - Y) - (t.ay - Y) * (t.bx - X);
    b0 = w0 / t.area;
    b1 = w1 / t.area;
    b2 = w2 / t.area;
    z = (b0 * t.az + b1 * t.bz) + b2 * t.cz;
    z = z == 0.f ? 0.f : z;
    return b0 >= 0.f && b1 >= 0.f && b2 >= 0.f && z >= 0.f;
}

__device__ __forceinline__ void rs_test(const RsTri& t, unsigned long long* __restrict__ keys, int64_t base, int i, int j, int W, float fh, float fw,
                                        uint32_t face)
{
    float z, b0, b1, b2;
    if (!rs_hit(t, rs_centre(j, fw), rs_centre(i, fh), z, b0, b1, b2)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | face;
    unsigned long long* p = keys + base + (int64_t)i * W + j;
    if (key < *p) atomicMin(p, key);
}

__global__ void __launch_bounds__(RS_THREADS) raster_setup_kernel(float4* __restrict__ screen, unsigned long long* __restrict__ keys,
                                                                  const float* __restrict__ verts, RsView vw, int V, int64_t n_vert, int64_t n_pix)
{
    const int64_t n = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (n < n_pix) keys[n] = RS_EMPTY;
    if (n < n_vert) {
        const int64_t bk = n / V;
        const int v = (int)(n - bk * V), k = (int)(bk % 3);
        const int64_t b = bk / 3;
        const float* p = verts + (b * V + v) * 3;
        const float x = p[0] * vw.scale[0] + vw.trans[0], y = p[1] * vw.scale[1] + vw.trans[1], z = p[2] * vw.scale[2] + vw.trans[2];
        float r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = (x * vw.rot[k][0][c] + y * vw.rot[k][1][c]) + z * vw.rot[k][2][c];
        screen[n] = make_float4(r[0], r[1], r[2] + vw.cam_dist, 0.f);
    }
}

__global__ void __launch_bounds__(RS_THREADS) raster_cover_kernel(unsigned long long* __restrict__ keys, const float4* __restrict__ screen,
                                                                  const int32_t* __restrict__ tris, int V, int F, int H, int W, int64_t n_tri)
{
    const int64_t n = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const float fh = (float)H, fw = (float)W;
    bool wide = false;
    if (n < n_tri) {
        const int64_t bv = n / F;
        const int f = (int)(n - bv * F);
        const RsTri t = rs_triangle(screen, tris, bv, f, V, H, W);
        const int bw = t.j1 - t.j0 + 1, bh = t.i1 - t.i0 + 1;
        if (bw > 0 && bh > 0) {
            wide = (int64_t)bw * bh > RS_BIG;
            if (!wide)
                for (int i = t.i0; i <= t.i1; ++i)
                    for (int j = t.j0; j <= t.j1; ++j) rs_test(t, keys, bv * H * W, i, j, W, fh, fw, (uint32_t)f);
        }
    }
    // the wave's wide triangles, one at a time, every lane on the same box
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t m = n - lane + l;          // < n_tri: lane l found it wide
        const int64_t bv = m / F;
        const int f = (int)(m - bv * F);
        const RsTri t = rs_triangle(screen, tris, bv, f, V, H, W);
        const int bw = t.j1 - t.j0 + 1;
        const int64_t cnt = (int64_t)bw * (t.i1 - t.i0 + 1);
        for (int64_t q = lane; q < cnt; q += 64) {
            const int di = (int)(q / bw), dj = (int)(q - (int64_t)di * bw);
            rs_test(t, keys, bv * H * W, t.i0 + di, t.j0 + dj, W, fh, fw, (uint32_t)f);
        }
    }
}

struct RsOut {
    int32_t* face;
    float* z;
    float* normal;
    uint8_t* render8;
    uint8_t* normal8;
    float* cond;
};

__device__ __forceinline__ float rs_depth(unsigned long long key) { return key == RS_EMPTY ? -1.f : __uint_as_float((uint32_t)(key >> 32)); }

__device__ __forceinline__ void rs_cross(float o[3], const float u[3], const float v[3])
{
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}

__device__ __forceinline__ void rs_normalize(float u[3])
{
    const float n = sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const float d = n < 1e-8f ? 1e-8f : n;
    u[0] = u[0] / d;
    u[1] = u[1] / d;
    u[2] = u[2] / d;
}

__global__ void __launch_bounds__(RS_THREADS) raster_resolve_kernel(RsOut out, const unsigned long long* __restrict__ keys,
                                                                    const float4* __restrict__ screen, const float* __restrict__ colors,
                                                                    const int32_t* __restrict__ tris, int V, int F, int H, int W, int tiles_x,
                                                                    int tiles_y, int64_t color_bstride, float dx, float dy)
{
    const int tid = threadIdx.x, lx = tid & (RS_TW - 1), ly = tid / RS_TW;
    const int tile = blockIdx.x, tx = tile % tiles_x, tr = tile / tiles_x, ty = tr % tiles_y;
    const int64_t bv = tr / tiles_y;
    const int j = tx * RS_TW + lx, i = ty * RS_TH + ly;
    if (j >= W || i >= H) return;          // no barrier and no wave operation below
    const int64_t hw = (int64_t)H * W, idx = bv * hw + (int64_t)i * W + j;          // < 3 B H W < 2^31
    const unsigned long long key = keys[idx];
    const bool covered = key != RS_EMPTY;
    const uint32_t fu = (uint32_t)key;
    const bool sane = covered && fu < (uint32_t)F;          // a key is written by the cover kernel alone: always true; keeps the reads in bounds
    const float D = rs_depth(key);
    float col[3] = {0.f, 0.f, 0.f};
    if (sane) {
        const int ia = tris[3 * (int64_t)fu + 0], ib = tris[3 * (int64_t)fu + 1], ic = tris[3 * (int64_t)fu + 2];
        if ((unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V) {
            RsTri t;
            rs_corners(t, screen + bv * V, ia, ib, ic);
            float z, b0, b1, b2;
            rs_hit(t, rs_centre(j, (float)W), rs_centre(i, (float)H), z, b0, b1, b2);
            const float* cb = colors + (bv / 3) * color_bstride;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = (b0 * cb[3 * (int64_t)ia + c] + b1 * cb[3 * (int64_t)ib + c]) + b2 * cb[3 * (int64_t)ic + c];
                v = v < 0.f ? 0.f : v;
                v = v > 255.f ? 255.f : v;
                col[c] = v != v ? 0.f : v;
            }
        }
    }
    uint32_t r8[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r8[c] = (uint32_t)(int)col[c];

    float nrm[3] = {0.f, 0.f, 0.f};
    if (i > 0 && i < H - 1 && j > 0 && j < W - 1) {
        const float De = rs_depth(keys[idx + 1]), Dw = rs_depth(keys[idx - 1]), Ds = rs_depth(keys[idx + W]), Dn = rs_depth(keys[idx - W]);
        const float px = (float)j * dx, py = (float)i * dy;
        const float vw[3] = {px - (float)(j + 1) * dx, py - py, D - De};
        const float vs[3] = {px - px, (float)(i + 1) * dy - py, Ds - D};
        const float ve[3] = {px - (float)(j - 1) * dx, py - py, D - Dw};
        const float vn[3] = {px - px, (float)(i - 1) * dy - py, Dn - D};
        float n1[3], n2[3];
        rs_cross(n1, vs, vw);
        rs_cross(n2, vn, ve);
        rs_normalize(n1);
        rs_normalize(n2);
        nrm[0] = n1[0] + n2[0];
        nrm[1] = n1[1] + n2[1];
        nrm[2] = n1[2] + n2[2];
        rs_normalize(nrm);
    }
    const bool keep = covered && r8[0] != 0 && r8[1] != 0 && r8[2] != 0;
    uint32_t n8[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) n8[c] = keep ? (uint32_t)(int)((nrm[c] + 1.f) * 127.5f) & 255u : 0u;

    if (out.face) out.face[idx] = covered ? (int32_t)fu : -1;
    if (out.z) out.z[idx] = D;
    if (out.normal) {
        out.normal[3 * idx + 0] = nrm[0];
        out.normal[3 * idx + 1] = nrm[1];
        out.normal[3 * idx + 2] = nrm[2];
    }
    if (out.render8) {
        out.render8[3 * idx + 0] = (uint8_t)r8[0];
        out.render8[3 * idx + 1] = (uint8_t)r8[1];
        out.render8[3 * idx + 2] = (uint8_t)r8[2];
    }
    if (out.normal8) {
        out.normal8[3 * idx + 0] = (uint8_t)n8[0];
        out.normal8[3 * idx + 1] = (uint8_t)n8[1];
        out.normal8[3 * idx + 2] = (uint8_t)n8[2];
    }
    if (out.cond) {
        float* c = out.cond + bv * 7 * hw + (int64_t)i * W + j;          // a wave writes 64 consecutive floats of each plane
        c[0 * hw] = (float)r8[0] / 255.f;
        c[1 * hw] = (float)r8[1] / 255.f;
        c[2 * hw] = (float)r8[2] / 255.f;
        c[3 * hw] = (float)n8[0] / 255.f;
        c[4 * hw] = (float)n8[1] / 255.f;
        c[5 * hw] = (float)n8[2] / 255.f;
        c[6 * hw] = (n8[0] | n8[1] | n8[2]) != 0 ? 1.f : 0.f;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
extern "C" int hav_raster_param(int which) { return which == 0 ? RS_TH : which == 1 ? RS_TW : which == 2 ? RS_BIG : 0; }

extern "C" int hav_raster_ortho_f32(int32_t* face, float* z, float* normal, uint8_t* render8, uint8_t* normal8, float* cond, uint64_t* keys,
                                    float* screen, const float* verts, const float* colors, const int32_t* tris, int B, int V, int F, int H, int W,
                                    int colors_batched, const float* view34, void* stream_)
{
    if (!keys || !screen || !verts || !colors || !tris || !view34 || B < 1 || V < 1 || F < 1 || H < 1 || W < 1) return HAV_EINVAL;
    if (!face && !z && !normal && !render8 && !normal8 && !cond) return HAV_EINVAL;
    if (((uintptr_t)screen & 15) != 0 || ((uintptr_t)keys & 7) != 0) return HAV_EINVAL;
    for (int k = 0; k < 34; ++k)
        if (!std::isfinite(view34[k])) return HAV_EINVAL;
    const int64_t n_pix = (int64_t)B * 3 * H * W, n_vert = (int64_t)B * 3 * V, n_tri = (int64_t)B * 3 * F;
    if (n_pix >= (1LL << 31)) return HAV_EINVAL;
    const int tiles_x = (W + RS_TW - 1) / RS_TW, tiles_y = (H + RS_TH - 1) / RS_TH;
    const int64_t tiles = (int64_t)B * 3 * tiles_x * tiles_y;
    const int64_t b_setup = ((n_pix > n_vert ? n_pix : n_vert) + RS_THREADS - 1) / RS_THREADS, b_cover = (n_tri + RS_THREADS - 1) / RS_THREADS;
    if (tiles >= (1LL << 31) || b_setup >= (1LL << 31) || b_cover >= (1LL << 31)) return HAV_EUNSUP;
    RsView vw;
    for (int k = 0; k < 3; ++k) { vw.scale[k] = view34[k]; vw.trans[k] = view34[3 + k]; }
    for (int k = 0; k < 27; ++k) (&vw.rot[0][0][0])[k] = view34[6 + k];
    vw.cam_dist = view34[33];
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(raster_setup_kernel, dim3((unsigned)b_setup), dim3(RS_THREADS), 0, stream, reinterpret_cast<float4*>(screen),
                       reinterpret_cast<unsigned long long*>(keys), verts, vw, V, n_vert, n_pix);
    HAV_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_cover_kernel, dim3((unsigned)b_cover), dim3(RS_THREADS), 0, stream, reinterpret_cast<unsigned long long*>(keys),
                       reinterpret_cast<const float4*>(screen), tris, V, F, H, W, n_tri);
    HAV_LAUNCH_CHECK();
    RsOut out = {face, z, normal, render8, normal8, cond};
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)tiles), dim3(RS_THREADS), 0, stream, out,
                       reinterpret_cast<const unsigned long long*>(keys), reinterpret_cast<const float4*>(screen), colors, tris, V, F, H, W, tiles_x,
                       tiles_y, colors_batched ? (int64_t)V * 3 : (int64_t)0, (float)(-2.0 / W), (float)(-2.0 / H));
    HAV_LAUNCH_CHECK();
    return 0;
}
