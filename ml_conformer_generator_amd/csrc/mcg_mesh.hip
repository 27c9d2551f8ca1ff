// Generalized winding number of a triangle mesh ("Solid references"): the inside / outside test, the
// density and the atom count behind a watertight mesh used as the reference shape.
//   w(p) = (1 / 4 pi) sum_f 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|),  a, b, c = v - p
// (van Oosterom and Strackee's solid angle of a triangle): +-1 inside a closed, consistently oriented surface, 0 outside.
//   k_mesh_winding:  one lane per point (an array, or the grid points of axes[3][n] in `mcg_shape::grid_point` order);
//                    triangles staged through LDS in tiles of MW_TILE, every lane reading the same triangle by broadcast.
//                    blockIdx.y = split s of S = mesh_splits(F), which walks tiles [s T / S, (s + 1) T / S).  S = 1 writes
//                    the result, S > 1 the split's partial sum to part[s][P], and
//   k_mesh_combine:  adds the partial sums in split order.
//   k_mesh_atoms_outside: one 64-lane workgroup per molecule, one lane per atom; walks the same splits one after the other
//                    and adds them in the same order, then counts.
// S and the tile ranges depend on F alone and every sum has one order, so w of a point has the same bits whatever the number
// of points, its place among them, array or grid mode, and in `mcg_mesh_atoms_outside`.  fp32, every multiply-add written
// out, contraction off.  No atomics.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"

#pragma clang fp contract(off)

namespace {

using mcg_shape::MAX_ATOMS;
using mcg_shape::atom_count;
using mcg_shape::grid_point;

constexpr int MW_TILE = 256;            // triangles per LDS tile
constexpr int MW_TILE_FLOATS = 12;      // a, b, c as three float4 (w unused): three 16-byte broadcast reads per triangle
constexpr int MW_SPLIT_TILES = 4;       // tiles per split, until MW_MAX_SPLITS splits are reached
constexpr int MW_MAX_SPLITS = 64;
constexpr float MW_INV_2PI = 0.15915494309189535f;

__host__ __device__ inline int mesh_tiles(int F) { return (F + MW_TILE - 1) / MW_TILE; }
__host__ __device__ inline int mesh_splits(int F) {
    const int s = (mesh_tiles(F) + MW_SPLIT_TILES - 1) / MW_SPLIT_TILES;
    return s < 1 ? 1 : (s > MW_MAX_SPLITS ? MW_MAX_SPLITS : s);
}

// atan2 term of one triangle (corners q[0..2], q[4..6], q[8..10]) seen from p.  A point on a corner: every product with
// that corner's zero vector is a zero, the denominator's first term is +0 and is added first, so the term is atan2(+-0, +0)
// = +-0, never NaN.
__device__ __forceinline__ float solid_angle_term(float px, float py, float pz, const float4 A, const float4 B,
                                                  const float4 C) {
    const float ax = A.x - px, ay = A.y - py, az = A.z - pz;
    const float bx = B.x - px, by = B.y - py, bz = B.z - pz;
    const float cx = C.x - px, cy = C.y - py, cz = C.z - pz;
    const float la = sqrtf(__builtin_fmaf(az, az, __builtin_fmaf(ay, ay, ax * ax)));
    const float lb = sqrtf(__builtin_fmaf(bz, bz, __builtin_fmaf(by, by, bx * bx)));
    const float lc = sqrtf(__builtin_fmaf(cz, cz, __builtin_fmaf(cy, cy, cx * cx)));
    const float nx = __builtin_fmaf(by, cz, -(bz * cy));
    const float ny = __builtin_fmaf(bz, cx, -(bx * cz));
    const float nz = __builtin_fmaf(bx, cy, -(by * cx));
    const float det = __builtin_fmaf(az, nz, __builtin_fmaf(ay, ny, ax * nx));
    const float ab = __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
    const float bc = __builtin_fmaf(bz, cz, __builtin_fmaf(by, cy, bx * cx));
    const float ca = __builtin_fmaf(cz, az, __builtin_fmaf(cy, ay, cx * ax));
    const float den = __builtin_fmaf(ca, lb, __builtin_fmaf(bc, la, __builtin_fmaf(ab, lc, (la * lb) * lc)));
    return atan2f(det, den);
}

// Sum of the terms of the triangles in tiles [t0, t1), in triangle order, for the point of this lane.  Every lane of the
// workgroup of THREADS lanes must call it (it stages the tiles); lanes with `live` false add nothing.
template <int THREADS>
__device__ __forceinline__ float split_sum(float px, float py, float pz, bool live, const float* __restrict__ tri, int F,
                                           int t0, int t1, float4* tile) {
    float acc = 0.f;
    float* flat = reinterpret_cast<float*>(tile);
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * MW_TILE, nj = min(MW_TILE, F - j0);
        __syncthreads();                                        // the previous tile is read by every lane
        for (int i = threadIdx.x; i < nj * 9; i += THREADS) {
            const int j = i / 9, k = i - j * 9;
            flat[j * MW_TILE_FLOATS + (k / 3) * 4 + k % 3] = tri[(size_t)j0 * 9 + i];
        }
        __syncthreads();
        if (live) {
#pragma unroll 2
            for (int j = 0; j < nj; ++j)
                acc += solid_angle_term(px, py, pz, tile[j * 3], tile[j * 3 + 1], tile[j * 3 + 2]);
        }
    }
    return acc;
}

__device__ __forceinline__ void split_range(int F, int s, int S, int* t0, int* t1) {
    const int T = mesh_tiles(F);
    *t0 = (int)((long)s * T / S);
    *t1 = (int)((long)(s + 1) * T / S);
}

// w from the sum of the atan2 terms; occupancy: the solid's density, 1 where |w| > 0.5 (NaN compares false: 0).
__device__ __forceinline__ float finish(float sum, bool bad, int occupancy) {
    const float w = bad ? __builtin_nanf("") : sum * MW_INV_2PI;
    return occupancy ? (fabsf(w) > 0.5f ? 1.f : 0.f) : w;
}

// points != nullptr: P points [P,3]; else the n^3 grid points of axes[3][n].  S = gridDim.y.
__global__ __launch_bounds__(MW_TILE) void k_mesh_winding(const float* __restrict__ tri, int F,
                                                          const float* __restrict__ points,
                                                          const float* __restrict__ axes, int n, long P, int occupancy,
                                                          float* __restrict__ out) {
    __shared__ float4 tile[MW_TILE * 3];
    const long a = (long)blockIdx.x * MW_TILE + threadIdx.x;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (a < P) {
        if (points != nullptr) {
            px = points[a * 3], py = points[a * 3 + 1], pz = points[a * 3 + 2];
        } else {
            const float3 p = grid_point(axes, n, (int)a);
            px = p.x, py = p.y, pz = p.z;
        }
    }
    const bool bad = !(isfinite(px) && isfinite(py) && isfinite(pz));
    const int S = gridDim.y;
    int t0, t1;
    split_range(F, blockIdx.y, S, &t0, &t1);
    const float sum = split_sum<MW_TILE>(px, py, pz, a < P && !bad, tri, F, t0, t1, tile);
    if (a >= P) return;
    if (S == 1) out[a] = finish(sum, bad, occupancy);
    else out[(size_t)blockIdx.y * P + a] = bad ? __builtin_nanf("") : sum;
}

__global__ __launch_bounds__(256) void k_mesh_combine(const float* __restrict__ part, long P, int S, int occupancy,
                                                      float* __restrict__ out) {
    for (long a = (long)blockIdx.x * 256 + threadIdx.x; a < P; a += (long)gridDim.x * 256) {
        float v = part[a];
        for (int s = 1; s < S; ++s) v += part[(size_t)s * P + a];
        out[a] = finish(v, isnan(v), occupancy);
    }
}

__global__ __launch_bounds__(MAX_ATOMS) void k_mesh_atoms_outside(const float* __restrict__ tri, int F,
                                                                  const float* __restrict__ posed,
                                                                  const int* __restrict__ n_nodes, int N,
                                                                  int* __restrict__ outside, float* __restrict__ w_out) {
    __shared__ float4 tile[MW_TILE * 3];
    const int b = blockIdx.x, i = threadIdx.x;
    const int na = atom_count(n_nodes[b], N);
    const bool real = i < na;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (real) {
        const float* x = posed + ((size_t)b * N + i) * 3;
        px = x[0], py = x[1], pz = x[2];
    }
    const bool bad = !(isfinite(px) && isfinite(py) && isfinite(pz));
    const int S = mesh_splits(F);
    float sum = 0.f;
    for (int s = 0; s < S; ++s) {
        int t0, t1;
        split_range(F, s, S, &t0, &t1);
        const float part = split_sum<MAX_ATOMS>(px, py, pz, real && !bad, tri, F, t0, t1, tile);
        sum = s == 0 ? part : sum + part;
    }
    const float w = finish(sum, bad, 0);
    if (w_out != nullptr && i < N) w_out[(size_t)b * N + i] = real ? w : 0.f;
    const int any_bad = __syncthreads_or(real && bad);
    const int count = __syncthreads_count(real && !(fabsf(w) > 0.5f));
    if (i == 0) outside[b] = any_bad ? -1 : count;
}

int launch_winding(const char* who, const float* tri, int F, const float* points, long P, const float* axes, int n,
                   int occupancy, float* out, float* partial_ws, void* stream) {
    const bool grid = points == nullptr;
    if (!tri || !out || F < 1 || F > MCG_MESH_MAX_FACES || (grid ? (!axes || n < 2 || n > MCG_MESH_MAX_N)
                                                                 : (P < 1 || P > MCG_MESH_MAX_POINTS)) ||
        (mesh_splits(F) > 1 && !partial_ws)) {
        mcg_set_error("%s: bad arguments (non-null buffers, 1 <= F <= %d, %s, partial_ws when mcg_mesh_splits(F) > 1)",
                      who, MCG_MESH_MAX_FACES, grid ? "2 <= n <= 256" : "1 <= P <= 2^24");
        return MCG_ERR_ARG;
    }
    if (grid) P = (long)n * n * n;
    hipStream_t s = (hipStream_t)stream;
    const int S = mesh_splits(F);
    const unsigned xb = (unsigned)((P + MW_TILE - 1) / MW_TILE);
    hipLaunchKernelGGL(k_mesh_winding, dim3(xb, S), dim3(MW_TILE), 0, s, tri, F, points, axes, n, P, occupancy,
                       S == 1 ? out : partial_ws);
    if (S > 1) {
        const long blocks = (P + 255) / 256;
        hipLaunchKernelGGL(k_mesh_combine, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, partial_ws, P,
                           S, occupancy, out);
    }
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

}  // namespace

extern "C" {

int mcg_mesh_splits(int F) { return F < 1 || F > MCG_MESH_MAX_FACES ? 0 : mesh_splits(F); }

int mcg_mesh_winding(const float* tri, int F, const float* points, int P, const float* axes, int n, float* w_out,
                     float* partial_ws, void* stream) {
    if ((points != nullptr) == (axes != nullptr)) {
        mcg_set_error("mcg_mesh_winding: bad arguments (either points[P,3] or axes[3,n], not both and not neither)");
        return MCG_ERR_ARG;
    }
    return launch_winding("mcg_mesh_winding", tri, F, points, P, axes, n, 0, w_out, partial_ws, stream);
}

int mcg_mesh_occupancy(const float* tri, int F, const float* axes, int n, float* f_out, float* partial_ws, void* stream) {
    if (!axes) {
        mcg_set_error("mcg_mesh_occupancy: bad arguments (axes is null)");
        return MCG_ERR_ARG;
    }
    return launch_winding("mcg_mesh_occupancy", tri, F, nullptr, 0, axes, n, 1, f_out, partial_ws, stream);
}

int mcg_mesh_atoms_outside(const float* tri, int F, const float* posed, const int32_t* n_nodes_dev, int B, int N,
                           int32_t* outside, float* w_out, void* stream) {
    if (!tri || !posed || !n_nodes_dev || !outside || F < 1 || F > MCG_MESH_MAX_FACES || B < 1 ||
        B > MCG_MESH_MAX_POINTS / MAX_ATOMS || N < 1 || N > MAX_ATOMS) {
        mcg_set_error("mcg_mesh_atoms_outside: bad arguments (non-null buffers, 1 <= F <= %d, 1 <= B <= %d, 1 <= N <= %d)",
                      MCG_MESH_MAX_FACES, MCG_MESH_MAX_POINTS / MAX_ATOMS, MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    hipLaunchKernelGGL(k_mesh_atoms_outside, dim3(B), dim3(MAX_ATOMS), 0, (hipStream_t)stream, tri, F, posed, n_nodes_dev, N,
                       outside, w_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

}  // extern "C"
