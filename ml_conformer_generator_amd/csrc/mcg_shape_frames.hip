// Principal shape frames of a padded batch (the frame half of `evaluate_samples`): the reference's
// `get_shape_quadrupole_for_molecule` (cheminformatics/shape_similarity.py:18-202) for B molecules of N <= 64 atoms.
//
// One workgroup of 1 024 lanes per molecule.  The neighbour graph (0 < d_ij < threshold, d the fp32 Euclidean distance,
// :233-266) is built ONCE per launch from the coordinates passed in: one 64-bit neighbour mask per atom, the edge list
// i < j, and per edge the mask of common neighbours above j (its third-member candidates).  Cliques are never stored:
//   order 1: lane = atom (strided), order 2: lane = edge (strided), orders >= 3: lane = triangle (strided over the
//   exclusive prefix of the per-edge candidate counts), and below each triangle a depth-first search over mask
//   intersections restricted to higher indices, one template level per order (registers only, no stack in memory).
// Per clique (`product_of_n_gaussians`, :205-230) the centre, gamma = sum|c|^2 - |sum c|^2 / k and the amplitude
// A^k exp(-alpha gamma) are fp32, the member sums run in index order; each lane sums the terms of ITS work items in fp64;
// the lanes are reduced in a fixed order (butterfly per wave, then the 16 wave partials in wave order).  The assignment
// of work to lanes depends only on the molecule's own atoms, so every result is bit-identical run to run and whatever
// the batch, row or padded width.  No atomics.
//   k_shape_moments: pass 1 (input points: volume, first moments -> shape centre), pass 2 (centred points: second-moment
//                    tensor / volume), optional exact clique counts per order.
//   k_shape_frames:  pass 3 on the centred points rotated by the host's eigenvectors: diagonal second moments, sorted
//                    descending, frame axes permuted to match (:143-202).  Optionally (`mcg_shape_frames_tf`) the rigid
//                    transform of the frame: M = V P (eigenvectors, then the axis permutation) and t = atom mean + shape
//                    centre, so that frames = (coords - t) @ M on the real rows.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own, as the reference's torch expressions

namespace {

using mcg_shape::MAX_ATOMS;
static_assert(MAX_ATOMS <= 64, "one 64-bit neighbour mask per atom");

constexpr int SF_MAX_TERMS = 8;
constexpr int SF_MAX_EDGES = MAX_ATOMS * (MAX_ATOMS - 1) / 2;
constexpr int SF_THREADS = 1024;
constexpr int SF_WAVES = SF_THREADS / 64;

// Per-order constants, computed on the host in double from the caller's alpha / amplitude and rounded to fp32 exactly as
// the reference's torch scalars are (`_shape_moments`): k = order.
struct ShapeTerms {
    float amp_k[SF_MAX_TERMS + 1];    // fl32(A^k)
    float vol_k[SF_MAX_TERMS + 1];    // fl32((pi / (k alpha))^1.5)
    float half_k[SF_MAX_TERMS + 1];   // fl32(1 / (2 k alpha))
    float amp1;                       // fl32(A): the single-atom amplitude
    float neg_alpha;                  // fl32(-alpha)
    float threshold;
    int n_terms;
    int centre_atoms;                 // subtract the atoms' mean before anything else
};

struct Shared {
    float px[MAX_ATOMS], py[MAX_ATOMS], pz[MAX_ATOMS], pq[MAX_ATOMS];   // points of the pass, |p|^2
    unsigned long long nbr[MAX_ATOMS];
    unsigned long long cand[SF_MAX_EDGES];       // per edge (i, j): neighbours of both above j
    unsigned int tri_start[SF_MAX_EDGES + 1];    // exclusive prefix of popcount(cand)
    unsigned short edge[SF_MAX_EDGES];           // i | j << 8
    int row_start[MAX_ATOMS + 1];
    double red[SF_WAVES][6];
    unsigned long long cred[SF_WAVES][SF_MAX_TERMS - 1];
    double sums[6];
    unsigned long long counts[SF_MAX_TERMS - 1];
    float mean[3];                               // the atoms' mean subtracted first (centre_atoms), else 0
    int n_edges;
};

__device__ __forceinline__ unsigned long long above(int i) { return i >= 63 ? 0ull : (~0ull << (i + 1)); }

// One term into the lane's fp64 sums.  PASS 1: volume + first moments; 2: diagonal + off-diagonal second moments; 3: diagonal.
template <int PASS>
__device__ __forceinline__ void add_term(double* a, float w, float cx, float cy, float cz, float h, bool neg) {
    float t[6];
    int nt;
    if constexpr (PASS == 1) {
        t[0] = w; t[1] = w * cx; t[2] = w * cy; t[3] = w * cz; nt = 4;
    } else {
        t[0] = w * (cx * cx + h); t[1] = w * (cy * cy + h); t[2] = w * (cz * cz + h); nt = 3;
        if constexpr (PASS == 2) { t[3] = w * (cx * cy); t[4] = w * (cx * cz); t[5] = w * (cy * cz); nt = 6; }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (k < nt) a[k] += neg ? -(double)t[k] : (double)t[k];
}

// A clique of order K from its member sums (index order): s = sum c, q = sum |c|^2.
template <int PASS, int K>
__device__ __forceinline__ void clique(double* a, unsigned* cnt, float sx, float sy, float sz, float q, const ShapeTerms& T) {
    const float kf = (float)K;
    const float gamma = q - ((sx * sx + sy * sy) + sz * sz) / kf;
    const float w = (T.amp_k[K] * expf(T.neg_alpha * gamma)) * T.vol_k[K];
    add_term<PASS>(a, w, sx / kf, sy / kf, sz / kf, T.half_k[K], (K & 1) == 0);
    if constexpr (PASS == 1) ++cnt[K - 2];
}

template <int PASS, int K>
__device__ void dfs(const Shared& s, unsigned long long cand, float sx, float sy, float sz, float q, const ShapeTerms& T,
                    double* a, unsigned* cnt) {
    do {
        const int v = __builtin_ctzll(cand);
        cand &= cand - 1;                          // what is left is above v
        const float nx = sx + s.px[v], ny = sy + s.py[v], nz = sz + s.pz[v], nq = q + s.pq[v];
        clique<PASS, K>(a, cnt, nx, ny, nz, nq, T);
        if constexpr (K < SF_MAX_TERMS) {
            if (K < T.n_terms) {
                const unsigned long long next = cand & s.nbr[v];
                if (next) dfs<PASS, K + 1>(s, next, nx, ny, nz, nq, T, a, cnt);
            }
        }
    } while (cand);
}

// Every clique of the molecule, each exactly once, on the lane its index assigns it to.
template <int PASS>
__device__ void enumerate(const Shared& s, int n, const ShapeTerms& T, double* a, unsigned* cnt) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += SF_THREADS)
        add_term<PASS>(a, T.amp1 * T.vol_k[1], s.px[i], s.py[i], s.pz[i], T.half_k[1], false);
    const int E = s.n_edges;
    for (int e = tid; e < E; e += SF_THREADS) {
        const int i = s.edge[e] & 0xff, j = s.edge[e] >> 8;
        clique<PASS, 2>(a, cnt, s.px[i] + s.px[j], s.py[i] + s.py[j], s.pz[i] + s.pz[j], s.pq[i] + s.pq[j], T);
    }
    if (T.n_terms < 3) return;
    const unsigned n_tri = s.tri_start[E];
    for (unsigned t = tid; t < n_tri; t += SF_THREADS) {
        int lo = 0, hi = E - 1;                    // the edge e with tri_start[e] <= t < tri_start[e + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s.tri_start[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const int e = lo, i = s.edge[e] & 0xff, j = s.edge[e] >> 8;
        unsigned long long m = s.cand[e];
        for (unsigned r = t - s.tri_start[e]; r; --r) m &= m - 1;
        const int k = __builtin_ctzll(m);
        const float sx = (s.px[i] + s.px[j]) + s.px[k], sy = (s.py[i] + s.py[j]) + s.py[k];
        const float sz = (s.pz[i] + s.pz[j]) + s.pz[k], q = (s.pq[i] + s.pq[j]) + s.pq[k];
        clique<PASS, 3>(a, cnt, sx, sy, sz, q, T);
        if (T.n_terms >= 4) {
            const unsigned long long next = (m & (m - 1)) & s.nbr[k];
            if (next) dfs<PASS, 4>(s, next, sx, sy, sz, q, T, a, cnt);
        }
    }
}

// Fixed-order block sums of the lanes' fp64 sums (and of the clique counts) into s.sums / s.counts.
template <int NA>
__device__ void reduce(Shared& s, double* a, const unsigned* cnt, bool with_counts) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        double v = a[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s.red[wid][k] = v;
    }
    if (with_counts) {
#pragma unroll
        for (int k = 0; k < SF_MAX_TERMS - 1; ++k) {
            unsigned long long v = cnt[k];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) s.cred[wid][k] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < NA) {
        double v = 0.0;
        for (int w = 0; w < SF_WAVES; ++w) v += s.red[w][threadIdx.x];
        s.sums[threadIdx.x] = v;
    } else if (with_counts && threadIdx.x >= 64 && threadIdx.x < 64 + SF_MAX_TERMS - 1) {
        unsigned long long v = 0;
        for (int w = 0; w < SF_WAVES; ++w) v += s.cred[w][threadIdx.x - 64];
        s.counts[threadIdx.x - 64] = v;
    }
    __syncthreads();
}

// Points of the molecule (optionally minus the atoms' mean) and its neighbour graph; returns n.
__device__ int load_and_build(Shared& s, const float* __restrict__ coords, const int32_t* __restrict__ n_nodes, int N,
                              const ShapeTerms& T) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), N);
    const float* x = coords + (size_t)b * N * 3;
    if (tid < n) { s.px[tid] = x[tid * 3]; s.py[tid] = x[tid * 3 + 1]; s.pz[tid] = x[tid * 3 + 2]; }
    __syncthreads();
    if (tid < 3) s.mean[tid] = 0.f;
    if (T.centre_atoms) {               // evaluate_shape's (x - mean) of the real atoms, summed in atom order
        float* mean = s.mean;
        if (tid < 3) {
            const float* p = tid == 0 ? s.px : tid == 1 ? s.py : s.pz;
            float acc = 0.f;
            for (int i = 0; i < n; ++i) acc += p[i];
            mean[tid] = acc / (float)max(n, 1);
        }
        __syncthreads();
        if (tid < n) { s.px[tid] -= mean[0]; s.py[tid] -= mean[1]; s.pz[tid] -= mean[2]; }
        __syncthreads();
    }
    if (tid < MAX_ATOMS) {
        unsigned long long m = 0;
        if (tid < n) {
            for (int j = 0; j < n; ++j) {
                const float dx = s.px[tid] - s.px[j], dy = s.py[tid] - s.py[j], dz = s.pz[tid] - s.pz[j];
                const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
                if (d < T.threshold && d > 0.f) m |= 1ull << j;
            }
            s.pq[tid] = (s.px[tid] * s.px[tid] + s.py[tid] * s.py[tid]) + s.pz[tid] * s.pz[tid];
        }
        s.nbr[tid] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < MAX_ATOMS; ++i) { s.row_start[i] = acc; acc += __popcll(s.nbr[i] & above(i)); }
        s.row_start[MAX_ATOMS] = acc;
        s.n_edges = acc;
    }
    __syncthreads();
    if (tid < n) {
        int e = s.row_start[tid];
        for (unsigned long long m = s.nbr[tid] & above(tid); m; m &= m - 1, ++e) {
            const int j = __builtin_ctzll(m);
            s.edge[e] = (unsigned short)(tid | (j << 8));
            s.cand[e] = s.nbr[tid] & s.nbr[j] & above(j);
        }
    }
    __syncthreads();
    if (tid < 64) {                     // exclusive prefix of the triangle counts: lane = contiguous chunk of edges
        const int E = s.n_edges, chunk = (E + 63) / 64, lo = min(tid * chunk, E), hi = min(lo + chunk, E);
        unsigned tot = 0;
        for (int e = lo; e < hi; ++e) tot += __popcll(s.cand[e]);
        unsigned inc = tot;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(inc, o, 64);
            if (tid >= o) inc += v;
        }
        unsigned run = inc - tot;
        for (int e = lo; e < hi; ++e) { s.tri_start[e] = run; run += __popcll(s.cand[e]); }
        if (tid == 63) s.tri_start[E] = inc;
    }
    __syncthreads();
    return n;
}

__global__ __launch_bounds__(SF_THREADS) void k_shape_moments(const float* __restrict__ coords,
                                                             const int32_t* __restrict__ n_nodes, int N, ShapeTerms T,
                                                             float* __restrict__ centre, float* __restrict__ tensor,
                                                             double* __restrict__ volume, int64_t* __restrict__ counts) {
    __shared__ Shared s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = load_and_build(s, coords, n_nodes, N, T);
    unsigned cnt[SF_MAX_TERMS - 1] = {0, 0, 0, 0, 0, 0, 0};
    {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        enumerate<1>(s, n, T, a, cnt);
        reduce<4>(s, a, cnt, counts != nullptr);
    }
    const double vol = s.sums[0];
    float c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = (float)(s.sums[1 + d] / vol);        // (first / vol).float()  (:86-89)
    if (tid == 0) {
        volume[b] = vol;
        for (int d = 0; d < 3; ++d) centre[b * 3 + d] = c[d];
    }
    if (counts != nullptr && tid < T.n_terms - 1) counts[(size_t)b * (T.n_terms - 1) + tid] = (int64_t)s.counts[tid];
    __syncthreads();
    if (tid < n) {
        const float x = s.px[tid] - c[0], y = s.py[tid] - c[1], z = s.pz[tid] - c[2];
        s.px[tid] = x; s.py[tid] = y; s.pz[tid] = z;
        s.pq[tid] = (x * x + y * y) + z * z;
    }
    __syncthreads();
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    enumerate<2>(s, n, T, a, cnt);
    reduce<6>(s, a, cnt, false);
    if (tid < 9) {                                  // _moment_tensor: ii / ij in fp32, over fp32(volume)
        const int r = tid / 3, col = tid % 3;
        const int idx = r == col ? r : (r + col == 1 ? 3 : (r + col == 2 ? 4 : 5));    // xy, xz, yz
        tensor[(size_t)b * 9 + tid] = (float)s.sums[idx] / (float)vol;
    }
}

__global__ __launch_bounds__(SF_THREADS) void k_shape_frames(const float* __restrict__ coords,
                                                            const int32_t* __restrict__ n_nodes, int N, ShapeTerms T,
                                                            const float* __restrict__ centre,
                                                            const float* __restrict__ eigvecs,
                                                            const double* __restrict__ volume,
                                                            float* __restrict__ moments, float* __restrict__ frames,
                                                            float* __restrict__ xform) {
    __shared__ Shared s;
    __shared__ int order[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = load_and_build(s, coords, n_nodes, N, T);          // the graph of the moments launch, rebuilt
    if (tid < n) {                                                   // (centred @ vecs)
        const float cx = s.px[tid] - centre[b * 3], cy = s.py[tid] - centre[b * 3 + 1], cz = s.pz[tid] - centre[b * 3 + 2];
        const float* V = eigvecs + (size_t)b * 9;
        float r[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) r[j] = fmaf(cz, V[6 + j], fmaf(cy, V[3 + j], cx * V[j]));
        s.px[tid] = r[0]; s.py[tid] = r[1]; s.pz[tid] = r[2];
        s.pq[tid] = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    }
    __syncthreads();
    unsigned cnt[SF_MAX_TERMS - 1] = {0, 0, 0, 0, 0, 0, 0};
    double a[3] = {0.0, 0.0, 0.0};
    enumerate<3>(s, n, T, a, cnt);
    reduce<3>(s, a, cnt, false);
    if (tid == 0) {
        const float vol = (float)volume[b];
        float m[3];
        int o[3] = {0, 1, 2};
        for (int d = 0; d < 3; ++d) m[d] = (float)s.sums[d] / vol;
        for (int i = 1; i < 3; ++i)                // stable descending sort of the three main moments
            for (int k = i; k > 0 && m[o[k]] > m[o[k - 1]]; --k) { const int t = o[k]; o[k] = o[k - 1]; o[k - 1] = t; }
        for (int d = 0; d < 3; ++d) { moments[b * 3 + d] = m[o[d]]; order[d] = o[d]; }
        if (xform != nullptr) {             // M[i][d] = V[i][o[d]], t = mean + centre
            const float* V = eigvecs + (size_t)b * 9;
            for (int i = 0; i < 3; ++i)
                for (int d = 0; d < 3; ++d) xform[(size_t)b * 12 + i * 3 + d] = V[i * 3 + o[d]];
            for (int d = 0; d < 3; ++d) xform[(size_t)b * 12 + 9 + d] = s.mean[d] + centre[b * 3 + d];
        }
    }
    __syncthreads();
    for (int i = tid; i < N; i += SF_THREADS) {
        float* f = frames + ((size_t)b * N + i) * 3;
        if (i < n) {
            const float r[3] = {s.px[i], s.py[i], s.pz[i]};
            f[0] = r[order[0]]; f[1] = r[order[1]]; f[2] = r[order[2]];
        } else {
            f[0] = f[1] = f[2] = 0.f;
        }
    }
}

int make_terms(double alpha, double amplitude, float threshold, int n_terms, int centre_atoms, ShapeTerms* T,
               const char* who) {
    if (!(alpha > 0.0) || !(amplitude > 0.0) || !(threshold > 0.f) || n_terms < 2 || n_terms > SF_MAX_TERMS) {
        mcg_set_error("%s: bad arguments (alpha, amplitude, threshold > 0; 2 <= n_terms <= %d)", who, SF_MAX_TERMS);
        return MCG_ERR_ARG;
    }
    for (int k = 0; k <= SF_MAX_TERMS; ++k) {
        const double a = k * alpha;
        T->amp_k[k] = (float)pow(amplitude, (double)k);
        T->vol_k[k] = k ? (float)pow(M_PI / a, 1.5) : 0.f;
        T->half_k[k] = k ? (float)(1.0 / (2.0 * a)) : 0.f;
    }
    T->amp1 = (float)amplitude;
    T->neg_alpha = (float)(-alpha);
    T->threshold = threshold;
    T->n_terms = n_terms;
    T->centre_atoms = centre_atoms ? 1 : 0;
    return MCG_OK;
}

int launch_frames(const float* coords, const int32_t* n_nodes_dev, int B, int N, const float* centre, const float* eigvecs,
                  const double* volume, double alpha, double amplitude, float neighbour_threshold, int n_terms,
                  int centre_atoms, float* moments, float* frames, float* xform, void* stream, const char* who) {
    ShapeTerms T;
    if (int rc = make_terms(alpha, amplitude, neighbour_threshold, n_terms, centre_atoms, &T, who)) return rc;
    hipLaunchKernelGGL(k_shape_frames, dim3(B), dim3(SF_THREADS), 0, (hipStream_t)stream, coords, n_nodes_dev, N, T, centre,
                       eigvecs, volume, moments, frames, xform);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

}  // namespace

extern "C" int mcg_shape_moments(const float* coords, const int32_t* n_nodes_dev, int B, int N, double alpha,
                                 double amplitude, float neighbour_threshold, int n_terms, int centre_atoms, float* centre,
                                 float* tensor, double* volume, int64_t* clique_counts, void* stream) {
    if (!coords || !n_nodes_dev || !centre || !tensor || !volume || B < 1 || N < 1 || N > MAX_ATOMS) {
        mcg_set_error("mcg_shape_moments: bad arguments (non-null buffers, B >= 1, 1 <= N <= %d)", MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    ShapeTerms T;
    if (int rc = make_terms(alpha, amplitude, neighbour_threshold, n_terms, centre_atoms, &T, "mcg_shape_moments")) return rc;
    hipLaunchKernelGGL(k_shape_moments, dim3(B), dim3(SF_THREADS), 0, (hipStream_t)stream, coords, n_nodes_dev, N, T, centre,
                       tensor, volume, clique_counts);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_shape_frames(const float* coords, const int32_t* n_nodes_dev, int B, int N, const float* centre,
                                const float* eigvecs, const double* volume, double alpha, double amplitude,
                                float neighbour_threshold, int n_terms, int centre_atoms, float* moments, float* frames,
                                void* stream) {
    if (!coords || !n_nodes_dev || !centre || !eigvecs || !volume || !moments || !frames || B < 1 || N < 1 ||
        N > MAX_ATOMS) {
        mcg_set_error("mcg_shape_frames: bad arguments (non-null buffers, B >= 1, 1 <= N <= %d)", MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    return launch_frames(coords, n_nodes_dev, B, N, centre, eigvecs, volume, alpha, amplitude, neighbour_threshold, n_terms,
                         centre_atoms, moments, frames, nullptr, stream, "mcg_shape_frames");
}

extern "C" int mcg_shape_frames_tf(const float* coords, const int32_t* n_nodes_dev, int B, int N, const float* centre,
                                   const float* eigvecs, const double* volume, double alpha, double amplitude,
                                   float neighbour_threshold, int n_terms, int centre_atoms, float* moments, float* frames,
                                   float* xform, void* stream) {
    if (!coords || !n_nodes_dev || !centre || !eigvecs || !volume || !moments || !frames || !xform || B < 1 || N < 1 ||
        N > MAX_ATOMS) {
        mcg_set_error("mcg_shape_frames_tf: bad arguments (non-null buffers, B >= 1, 1 <= N <= %d)", MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    return launch_frames(coords, n_nodes_dev, B, N, centre, eigvecs, volume, alpha, amplitude, neighbour_threshold, n_terms,
                         centre_atoms, moments, frames, xform, stream, "mcg_shape_frames_tf");
}
