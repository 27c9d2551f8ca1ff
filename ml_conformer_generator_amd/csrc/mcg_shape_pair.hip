// Pairwise shape Tanimoto of B molecules placed in one common frame ("shape diversity"): all the
// pairwise overlaps on the reference's grid are one Gram matrix G = F F^T of the molecules' grid densities F[B, Gp].
//   k_pair_density:  F[b][g] = the density of molecule b at grid point g of the reference's grid, its atoms mapped into the
//                    reference's principal frame (y = (x - t_r) @ M_r) and staged in LDS, then `mcg_shape::density_at`
//                    (the bits `k_shape_density` gives for the same points).  NaN over the whole row of a molecule with no
//                    atoms or a non-finite coordinate; zero on the padded columns n^3 <= g < Gp.
//   k_pair_gram:     G on v_mfma_f32_16x16x4_f32 (exact fp32), tiles on or above the diagonal only, each value written to
//                    (i, j) and (j, i).  Determinism: the k order of every element is fixed by Gp alone.  Gp is split into
//                    PAIR_KSPLIT equal ranges, one per wave of the workgroup; a wave walks its range in blocks of 32, lane
//                    group q holding k = k0 + 8q .. k0 + 8q + 7 of its rows (two 16-byte loads), so sub-step s of a block
//                    sums k0 + s, k0 + 8 + s, k0 + 16 + s, k0 + 24 + s as one k-ordered fmaf chain; the four range sums are
//                    combined as (p0 + p1) + (p2 + p3) through LDS.  No atomics; the tile size (16, 32 or 64 rows) only
//                    decides which workgroup computes an element, never how.
//   k_pair_tanimoto: T_ij = G_ij / ((G_ii + G_jj) - G_ij): symmetric, and exactly 1 where G_ij = G_ii = G_jj.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"

#include <stdlib.h>

namespace {

using mcg_shape::MAX_ATOMS;
using mcg_shape::atom_count;
using mcg_shape::density_at;
using mcg_shape::grid_point;
using mcg_shape::rotate_row;

constexpr int PAIR_KSPLIT = 4;                                   // k ranges = waves per Gram workgroup
constexpr int PAIR_KBLOCK = 32;                                  // k per wave per block (4 lane groups x 8)
static_assert(MCG_SHAPE_PAIR_KALIGN == PAIR_KSPLIT * PAIR_KBLOCK, "Gp granularity");
constexpr int DENS_POINTS = 2048;                                // grid points per density workgroup (8 per lane)

// xform = M_r row-major [9], then t_r [3]: the reference's frame is (x - t_r) @ M_r (mcg_shape_frames_tf).
__global__ __launch_bounds__(256) void k_pair_density(const float* __restrict__ coords, const int* __restrict__ n_nodes,
                                                      int N, const float* __restrict__ ref_xform,
                                                      const float* __restrict__ axes, int n, float alpha, float amp,
                                                      int Gp, float* __restrict__ F) {
    __shared__ float c[MAX_ATOMS][3];
    __shared__ float m[12];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int na = atom_count(n_nodes[b], N);
    if (tid < 12) m[tid] = ref_xform[tid];
    __syncthreads();
    bool bad = false;
    for (int i = tid; i < na; i += 256) {
        const float* x = coords + ((size_t)b * N + i) * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
        bad |= !(isfinite(x0) && isfinite(x1) && isfinite(x2));
        rotate_row(x0 - m[9], x1 - m[10], x2 - m[11], m, c[i]);
    }
    const bool row_bad = __syncthreads_or(bad) != 0 || na == 0;
    const int total = n * n * n;
    const int end = min(Gp, (int)(blockIdx.x + 1) * DENS_POINTS);
    float* out = F + (size_t)b * Gp;
    for (int idx = blockIdx.x * DENS_POINTS + tid; idx < end; idx += 256) {
        float v = 0.f;
        if (idx < total) {
            const float3 p = grid_point(axes, n, idx);
            v = row_bad ? __builtin_nanf("") : density_at(p.x, p.y, p.z, c, na, alpha, amp);
        }
        out[idx] = v;
    }
}

// One workgroup per tile pair (I, J), I <= J, of T = 16 RT rows; wave w sums k range w of every element of the tile.
template <int RT>
__global__ __launch_bounds__(256) void k_pair_gram(const float* __restrict__ F, int B, int Gp, int nt,
                                                   float* __restrict__ G) {
    constexpr int T = 16 * RT;
    __shared__ float part[PAIR_KSPLIT][T * T];
    int t = blockIdx.x, I = 0;
    while (t >= nt - I) { t -= nt - I; ++I; }                    // row I of the upper triangle holds nt - I tiles
    const int J = I + t;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, q = lane >> 4;
    const float* ar[RT];
    const float* br[RT];
#pragma unroll
    for (int m = 0; m < RT; ++m) {                               // rows past B read row B - 1; their results are dropped
        ar[m] = F + (size_t)min(I * T + 16 * m + li, B - 1) * Gp + 8 * q;
        br[m] = F + (size_t)min(J * T + 16 * m + li, B - 1) * Gp + 8 * q;
    }
    const int kw = Gp / PAIR_KSPLIT;
    f32x4 acc[RT][RT];
#pragma unroll
    for (int m = 0; m < RT; ++m)
#pragma unroll
        for (int p = 0; p < RT; ++p) acc[m][p] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k = w * kw, k1 = k + kw; k < k1; k += PAIR_KBLOCK) {
        float a[RT][8], bv[RT][8];
#pragma unroll
        for (int m = 0; m < RT; ++m) {
            const float4 a0 = *(const float4*)(ar[m] + k), a1 = *(const float4*)(ar[m] + k + 4);
            const float4 b0 = *(const float4*)(br[m] + k), b1 = *(const float4*)(br[m] + k + 4);
            a[m][0] = a0.x; a[m][1] = a0.y; a[m][2] = a0.z; a[m][3] = a0.w;
            a[m][4] = a1.x; a[m][5] = a1.y; a[m][6] = a1.z; a[m][7] = a1.w;
            bv[m][0] = b0.x; bv[m][1] = b0.y; bv[m][2] = b0.z; bv[m][3] = b0.w;
            bv[m][4] = b1.x; bv[m][5] = b1.y; bv[m][6] = b1.z; bv[m][7] = b1.w;
        }
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int m = 0; m < RT; ++m)
#pragma unroll
                for (int p = 0; p < RT; ++p) acc[m][p] = mcg_mfma(a[m][s], bv[p][s], acc[m][p]);
    }
    // lane (li, q), register r of acc[m][p] = G[I T + 16 m + 4 q + r][J T + 16 p + li]
#pragma unroll
    for (int m = 0; m < RT; ++m)
#pragma unroll
        for (int p = 0; p < RT; ++p)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[w][(16 * m + 4 * q + r) * T + 16 * p + li] = acc[m][p][r];
    __syncthreads();
    for (int e = threadIdx.x; e < T * T; e += 256) {
        const int r = e / T, cc = e % T;
        const int i = I * T + r, j = J * T + cc;
        if (i >= B || j >= B || (I == J && r > cc)) continue;   // the diagonal tile writes from its upper half
        const float v = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
        G[(size_t)i * B + j] = v;
        G[(size_t)j * B + i] = v;
    }
}

__global__ __launch_bounds__(256) void k_pair_tanimoto(const float* __restrict__ G, int B, float* __restrict__ T) {
    const size_t total = (size_t)B * B;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t i = idx / B, j = idx % B;
        const float g = G[idx];
        T[idx] = g / ((G[i * B + i] + G[j * B + j]) - g);
    }
}

// Rows per wave tile side (RT = 1, 2 or 4 16-row tiles): the largest that still gives every CU two workgroups.
// MCG_SHAPE_PAIR_TILE=1|2|4 forces one (measurement only: the results are the same bits whichever runs).
int pick_tile(int B) {
    if (const char* e = getenv("MCG_SHAPE_PAIR_TILE")) {
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4) return v;
    }
    auto tiles = [B](int rt) { const long nt = (B + 16 * rt - 1) / (16 * rt); return nt * (nt + 1) / 2; };
    if (tiles(4) >= 512) return 4;
    if (tiles(2) >= 512) return 2;
    return 1;
}

template <int RT>
void launch_gram(const float* F, int B, int Gp, float* G, hipStream_t s) {
    const int nt = (B + 16 * RT - 1) / (16 * RT);
    hipLaunchKernelGGL(k_pair_gram<RT>, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, F, B, Gp, nt, G);
}

}  // namespace

extern "C" int mcg_shape_pair_tanimoto(const float* coords, const int32_t* n_nodes_dev, int B, int N,
                                       const float* ref_xform, const float* axes, int n, float alpha, float amplitude,
                                       float* density_ws, float* gram_ws, float* tanimoto, void* stream) {
    if (!coords || !n_nodes_dev || !ref_xform || !axes || !density_ws || !gram_ws || !tanimoto || B < 1 ||
        B > MCG_SHAPE_PAIR_MAX_B || N < 1 || N > MAX_ATOMS || n < 2 || n > MCG_SHAPE_PAIR_MAX_N) {
        mcg_set_error("mcg_shape_pair_tanimoto: bad arguments (non-null buffers, 1 <= B <= %d, 1 <= N <= %d, "
                      "2 <= n <= %d)", MCG_SHAPE_PAIR_MAX_B, MAX_ATOMS, MCG_SHAPE_PAIR_MAX_N);
        return MCG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int total = n * n * n;
    const int Gp = (total + MCG_SHAPE_PAIR_KALIGN - 1) / MCG_SHAPE_PAIR_KALIGN * MCG_SHAPE_PAIR_KALIGN;
    hipLaunchKernelGGL(k_pair_density, dim3((Gp + DENS_POINTS - 1) / DENS_POINTS, B), dim3(256), 0, s, coords, n_nodes_dev,
                       N, ref_xform, axes, n, alpha, amplitude, Gp, density_ws);
    switch (pick_tile(B)) {
        case 4: launch_gram<4>(density_ws, B, Gp, gram_ws, s); break;
        case 2: launch_gram<2>(density_ws, B, Gp, gram_ws, s); break;
        default: launch_gram<1>(density_ws, B, Gp, gram_ws, s); break;
    }
    const size_t pairs = (size_t)B * B;
    hipLaunchKernelGGL(k_pair_tanimoto, dim3((unsigned)((pairs + 255) / 256 < 8192 ? (pairs + 255) / 256 : 8192)), dim3(256), 0, s,
                       gram_ws, B, tanimoto);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
