// hav_isosurface.hip -- iso-surface of a scalar lattice by marching tetrahedra on the Kuhn subdivision, gfx950: the extractor behind
// havatar_amd.geometry.isosurface (native/iso_ops.py).  No reference counterpart: the reference writes no surface.
//
// Definition (include/havatar.h states it in full; geometry.py states it on ATen, tests/test_isosurface_cpu.py in plain loops).
//   f [D0,D1,D2] contiguous float32, n = (i D1 + j) D2 + k; a point is inside iff f > iso (strict; NaN is outside).
//   Lattice point n owns the seven edges n -> n + d, d in {0,1}^3 \ {0}, e = 4 di + 2 dj + dk - 1.  An owned edge whose far end is in the
//   grid and whose ends differ in inside-ness carries one vertex at t = (iso - f[n]) / (f[n+d] - f[n]) (float32; 0.5 when not finite, else
//   clamped to [0,1]).  Vertices are ordered by n, then e.
//   The cube at n (all of i < D0-1, j < D1-1, k < D2-1) splits into the six tetrahedra c0 = n, c1 = c0 + e_a1, c2 = c1 + e_a2, c3 = c2 + e_a3,
//   (a1,a2,a3) the permutations of (0,1,2) in lexicographic order.  One inside corner or one outside corner gives a triangle, two give two;
//   the order of a triangle's last two entries is a function of (tetrahedron, case) alone.  Triangles are ordered by n, tetrahedron, slot.
//
//   iso_classify_kernel  a 256-thread workgroup owns 256 consecutive n (k fastest: the corner loads of a wave are row-contiguous).  A thread
//                        loads its cube's corners, forms code = crossing mask (bits 0-6) | triangle count << 8 | corner inside bits << 16,
//                        and the workgroup adds the packed counts (vertices <= 7 x 256 in the low half, triangles <= 12 x 256 in the high
//                        half of one 32-bit word): one wave64 shuffle scan plus one LDS step across the four waves.
//   iso_vbase_kernel     the same scan of the codes, exclusive, plus the workgroup's vertex offset: vbase[n], a point's first vertex index.
//   iso_emit_kernel      the scan once more for the triangle offset; a thread writes its point's vertices (and normals) and its cube's
//                        triangles.  A triangle's vertex on the edge owned by lattice point p is vbase[p] + popcount(mask_p & ((1 << e) - 1)).
// The (tetrahedron, case) -> edges table is generated at compile time from the definition (iso_make_tab) and lives in __constant__ memory.
// No atomics, no allocation, no synchronisation, no environment reads: the same inputs give the same bits, and the launches can be captured.
// Every element of verts / normals [0,V) and tris [0,T) is written exactly once and nothing beyond.  LDS: 16 bytes per workgroup.
#include "hav_common.h"

#include <cmath>

#define ISO_P 256                            // lattice points (threads) per workgroup

// ---- the table: generated from the definition ----------------------------------------------------------------------------------------
// corner c of tetrahedron tau as a cube-corner offset 4 di + 2 dj + dk (axis a sets bit 4 >> a)
__host__ __device__ constexpr int iso_corner(int tau, int c)
{
    int a1 = 0, a2 = 0, cnt = 0;
    for (int x = 0; x < 3; ++x)
        for (int y = 0; y < 3; ++y)
            if (y != x) {          // ascending loops: lexicographic order of (a1, a2, a3)
                if (cnt == tau) { a1 = x; a2 = y; }
                ++cnt;
            }
    return c == 0 ? 0 : c == 1 ? (4 >> a1) : c == 2 ? ((4 >> a1) | (4 >> a2)) : 7;
}

struct IsoTab {
    uint8_t cnt[6 * 16];                     // triangles of (tau, case); case bit c = corner c inside
    uint8_t vert[6 * 16][2][3];              // (owner corner offset << 3) | e of each triangle entry, winding applied
};

constexpr IsoTab iso_make_tab()
{
    IsoTab t{};
    for (int tau = 0; tau < 6; ++tau)
        for (int cs = 0; cs < 16; ++cs) {
            int I[4] = {0, 0, 0, 0}, O[4] = {0, 0, 0, 0}, nI = 0, nO = 0;
            for (int c = 0; c < 4; ++c) {
                if ((cs >> c) & 1) I[nI++] = c;
                else O[nO++] = c;
            }
            int tri[2][3][2] = {};          // [slot][entry] = (p, q) corner pair
            int nt = 0;
            if (nI == 1) {
                nt = 1;
                for (int v = 0; v < 3; ++v) { tri[0][v][0] = I[0]; tri[0][v][1] = O[v]; }
            } else if (nI == 3) {
                nt = 1;
                for (int v = 0; v < 3; ++v) { tri[0][v][0] = O[0]; tri[0][v][1] = I[v]; }
            } else if (nI == 2) {
                nt = 2;
                tri[0][0][0] = I[0]; tri[0][0][1] = O[0];
                tri[0][1][0] = I[0]; tri[0][1][1] = O[1];
                tri[0][2][0] = I[1]; tri[0][2][1] = O[1];
                tri[1][0][0] = I[0]; tri[1][0][1] = O[0];
                tri[1][1][0] = I[1]; tri[1][1][1] = O[1];
                tri[1][2][0] = I[1]; tri[1][2][1] = O[0];
            }
            t.cnt[tau * 16 + cs] = (uint8_t)nt;
            // inside -> outside direction, scaled by nI nO > 0: nI sum(O) - nO sum(I), corner positions in index space
            int dir[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) {
                int sI = 0, sO = 0;
                for (int q = 0; q < nI; ++q) sI += (iso_corner(tau, I[q]) >> (2 - a)) & 1;
                for (int q = 0; q < nO; ++q) sO += (iso_corner(tau, O[q]) >> (2 - a)) & 1;
                dir[a] = nI * sO - nO * sI;
            }
            for (int s = 0; s < nt; ++s) {
                int m[3][3] = {};          // twice the edge midpoints
                for (int v = 0; v < 3; ++v)
                    for (int a = 0; a < 3; ++a)
                        m[v][a] = ((iso_corner(tau, tri[s][v][0]) >> (2 - a)) & 1) + ((iso_corner(tau, tri[s][v][1]) >> (2 - a)) & 1);
                int u[3] = {0, 0, 0}, w[3] = {0, 0, 0};
                for (int a = 0; a < 3; ++a) { u[a] = m[1][a] - m[0][a]; w[a] = m[2][a] - m[0][a]; }
                const int nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
                const bool flip = nx * dir[0] + ny * dir[1] + nz * dir[2] < 0;
                for (int v = 0; v < 3; ++v) {
                    const int src = (flip && v > 0) ? 3 - v : v;
                    const int p = tri[s][src][0], q = tri[s][src][1];
                    const int lo = iso_corner(tau, p < q ? p : q), hi = iso_corner(tau, p < q ? q : p);          // offsets nest: lo is a subset of hi
                    t.vert[tau * 16 + cs][s][v] = (uint8_t)((lo << 3) | ((hi ^ lo) - 1));
                }
            }
        }
    return t;
}

__constant__ IsoTab ISO_TAB = iso_make_tab();

struct IsoVec3 { float v[3]; };

// ---- the workgroup scan --------------------------------------------------------------------------------------------------------------
// exclusive prefix of the packed counts over the 256 threads, and their sum; every thread of the workgroup calls it
__device__ __forceinline__ uint32_t iso_block_scan(uint32_t w, uint32_t* total, uint32_t* sW)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = w;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) sW[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < ISO_P / 64; ++q) {
        const uint32_t s = sW[q];
        if (q < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - w;
}

__device__ __forceinline__ uint32_t iso_packed_counts(uint32_t code) { return (uint32_t)__popc(code & 0x7fu) | (((code >> 8) & 0xfu) << 16); }

__device__ __forceinline__ int iso_case(uint32_t bits, int tau)
{
    return (int)((bits & 1u) | (((bits >> iso_corner(tau, 1)) & 1u) << 1) | (((bits >> iso_corner(tau, 2)) & 1u) << 2) | (((bits >> 7) & 1u) << 3));
}

// ---- classify ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ISO_P) iso_classify_kernel(uint32_t* __restrict__ codes, int32_t* __restrict__ block_counts,
                                                             const float* __restrict__ f, int D0, int D1, int D2, int N, float iso)
{
    __shared__ uint32_t sW[ISO_P / 64];
    const int64_t n64 = (int64_t)blockIdx.x * ISO_P + threadIdx.x;
    uint32_t w = 0;
    if (n64 < N) {
        const int n = (int)n64;
        const int k = n % D2, r = n / D2, j = r % D1, i = r / D1;
        const int s0 = D1 * D2;
        const bool hi = i + 1 < D0, hj = j + 1 < D1, hk = k + 1 < D2;
        const bool in0 = f[n] > iso;
        uint32_t bits = in0 ? 1u : 0u, mask = 0;
#pragma unroll
        for (int off = 1; off < 8; ++off) {
            const int di = (off >> 2) & 1, dj = (off >> 1) & 1, dk = off & 1;
            if ((!di || hi) && (!dj || hj) && (!dk || hk)) {
                const bool in = f[n + di * s0 + dj * D2 + dk] > iso;
                bits |= (in ? 1u : 0u) << off;
                if (in != in0) mask |= 1u << (off - 1);
            }
        }
        uint32_t nt = 0;
        if (hi && hj && hk) {
#pragma unroll
            for (int tau = 0; tau < 6; ++tau) {
                const int pc = __popc((uint32_t)iso_case(bits, tau));
                nt += pc == 2 ? 2u : (pc == 1 || pc == 3) ? 1u : 0u;
            }
        }
        const uint32_t code = mask | (nt << 8) | (bits << 16);
        codes[n] = code;
        w = iso_packed_counts(code);
    }
    uint32_t total;
    iso_block_scan(w, &total, sW);
    if (threadIdx.x == 0) {
        block_counts[2 * (int64_t)blockIdx.x] = (int32_t)(total & 0xffffu);
        block_counts[2 * (int64_t)blockIdx.x + 1] = (int32_t)(total >> 16);
    }
}

// ---- emit, first launch: a point's first vertex index ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(ISO_P) iso_vbase_kernel(int32_t* __restrict__ vbase, const uint32_t* __restrict__ codes,
                                                          const int32_t* __restrict__ block_offsets, int N)
{
    __shared__ uint32_t sW[ISO_P / 64];
    const int64_t n64 = (int64_t)blockIdx.x * ISO_P + threadIdx.x;
    const bool live = n64 < N;
    uint32_t total;
    const uint32_t excl = iso_block_scan(live ? iso_packed_counts(codes[n64]) : 0u, &total, sW);
    if (live) vbase[n64] = block_offsets[2 * (int64_t)blockIdx.x] + (int32_t)(excl & 0xffffu);
}

// ---- emit, second launch ---------------------------------------------------------------------------------------------------------------
// central difference of f at lattice point p = (i,j,k), one-sided at a grid face, each axis divided by its spacing
__device__ __forceinline__ void iso_grad(float g[3], const float* __restrict__ f, int p, int i, int j, int k, int D0, int D1, int D2, int s0,
                                         const IsoVec3& h)
{
    const int idx[3] = {i, j, k}, dim[3] = {D0, D1, D2}, st[3] = {s0, D2, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool lo = idx[a] > 0, up = idx[a] + 1 < dim[a];
        const float fm = f[lo ? p - st[a] : p], fp = f[up ? p + st[a] : p];
        g[a] = (fp - fm) / ((lo && up) ? 2.f * h.v[a] : h.v[a]);
    }
}

template <bool NRM>
__global__ void __launch_bounds__(ISO_P) iso_emit_kernel(float* __restrict__ verts, float* __restrict__ normals, int32_t* __restrict__ tris,
                                                         const int32_t* __restrict__ vbase, const uint32_t* __restrict__ codes,
                                                         const int32_t* __restrict__ block_offsets, const float* __restrict__ f, int D0,
                                                         int D1, int D2, int N, float iso, IsoVec3 origin, IsoVec3 spacing)
{
    __shared__ uint32_t sW[ISO_P / 64];
    const int64_t n64 = (int64_t)blockIdx.x * ISO_P + threadIdx.x;
    const bool live = n64 < N;
    const uint32_t code = live ? codes[n64] : 0u;
    uint32_t total;
    const uint32_t excl = iso_block_scan(iso_packed_counts(code), &total, sW);
    if (!live) return;
    const int n = (int)n64;
    const int k = n % D2, r = n / D2, j = r % D1, i = r / D1;
    const int s0 = D1 * D2;
    const uint32_t mask = code & 0x7fu, nt = (code >> 8) & 0xfu;

    if (mask) {
        const float a = f[n];
        float g0[3];
        if constexpr (NRM) iso_grad(g0, f, n, i, j, k, D0, D1, D2, s0, spacing);
        int64_t v = vbase[n];
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            if (!((mask >> e) & 1u)) continue;
            const int off = e + 1;
            const int di = (off >> 2) & 1, dj = (off >> 1) & 1, dk = off & 1;
            const int p = n + di * s0 + dj * D2 + dk;
            const float b = f[p];
            float t = (iso - a) / (b - a);
            t = std::isfinite(t) ? fminf(fmaxf(t, 0.f), 1.f) : 0.5f;
            verts[3 * v + 0] = origin.v[0] + ((float)i + t * (float)di) * spacing.v[0];
            verts[3 * v + 1] = origin.v[1] + ((float)j + t * (float)dj) * spacing.v[1];
            verts[3 * v + 2] = origin.v[2] + ((float)k + t * (float)dk) * spacing.v[2];
            if constexpr (NRM) {
                float g1[3];
                iso_grad(g1, f, p, i + di, j + dj, k + dk, D0, D1, D2, s0, spacing);
                const float x = -(g0[0] + t * (g1[0] - g0[0])), y = -(g0[1] + t * (g1[1] - g0[1])), z = -(g0[2] + t * (g1[2] - g0[2]));
                const float len = sqrtf(x * x + y * y + z * z);
                const bool ok = std::isfinite(len) && len > 0.f;
                normals[3 * v + 0] = ok ? x / len : 0.f;
                normals[3 * v + 1] = ok ? y / len : 0.f;
                normals[3 * v + 2] = ok ? z / len : 0.f;
            }
            ++v;
        }
    }

    if (nt) {
        const uint32_t bits = (code >> 16) & 0xffu;
        int64_t t = (int64_t)block_offsets[2 * (int64_t)blockIdx.x + 1] + (int64_t)(excl >> 16);
#pragma unroll
        for (int tau = 0; tau < 6; ++tau) {
            const int ent = tau * 16 + iso_case(bits, tau);
            const int cnt = ISO_TAB.cnt[ent];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s >= cnt) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int pv = ISO_TAB.vert[ent][s][c];
                    const int off = pv >> 3, e = pv & 7;
                    const int p = n + ((off >> 2) & 1) * s0 + ((off >> 1) & 1) * D2 + (off & 1);          // a corner of an existing cube: in the grid
                    tris[3 * t + c] = vbase[p] + __popc(codes[p] & ((1u << e) - 1u));
                }
                ++t;
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static int iso_size(int D0, int D1, int D2, int64_t* N, int64_t* blocks)
{
    if (D0 < 2 || D1 < 2 || D2 < 2) return HAV_EINVAL;
    *N = (int64_t)D0 * D1 * D2;
    if (*N >= (1LL << 31)) return HAV_EUNSUP;
    *blocks = (*N + ISO_P - 1) / ISO_P;
    if (*blocks > 0x7fffffffLL) return HAV_EUNSUP;
    return 0;
}

extern "C" int64_t hav_iso_blocks(int D0, int D1, int D2)
{
    int64_t N, blocks;
    return iso_size(D0, D1, D2, &N, &blocks) == 0 ? blocks : 0;
}

extern "C" int hav_iso_classify(uint32_t* codes, int32_t* block_counts, const float* f, int D0, int D1, int D2, float iso, void* stream_)
{
    if (!codes || !block_counts || !f || !std::isfinite(iso)) return HAV_EINVAL;
    int64_t N, blocks;
    const int rc = iso_size(D0, D1, D2, &N, &blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(iso_classify_kernel, dim3((unsigned)blocks), dim3(ISO_P), 0, (hipStream_t)stream_, codes, block_counts, f, D0, D1, D2,
                       (int)N, iso);
    HAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int hav_iso_emit(float* verts, float* normals, int32_t* tris, int32_t* vbase, const uint32_t* codes, const int32_t* block_offsets,
                            const float* f, int D0, int D1, int D2, float iso, const float origin[3], const float spacing[3], void* stream_)
{
    if (!verts || !tris || !vbase || !codes || !block_offsets || !f || !origin || !spacing || !std::isfinite(iso)) return HAV_EINVAL;
    int64_t N, blocks;
    const int rc = iso_size(D0, D1, D2, &N, &blocks);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    IsoVec3 o, h;
    for (int a = 0; a < 3; ++a) { o.v[a] = origin[a]; h.v[a] = spacing[a]; }
    hipLaunchKernelGGL(iso_vbase_kernel, dim3((unsigned)blocks), dim3(ISO_P), 0, stream, vbase, codes, block_offsets, (int)N);
    HAV_LAUNCH_CHECK();
    if (normals)
        hipLaunchKernelGGL((iso_emit_kernel<true>), dim3((unsigned)blocks), dim3(ISO_P), 0, stream, verts, normals, tris, vbase, codes,
                           block_offsets, f, D0, D1, D2, (int)N, iso, o, h);
    else
        hipLaunchKernelGGL((iso_emit_kernel<false>), dim3((unsigned)blocks), dim3(ISO_P), 0, stream, verts, normals, tris, vbase, codes,
                           block_offsets, f, D0, D1, D2, (int)N, iso, o, h);
    HAV_LAUNCH_CHECK();
    return 0;
}
