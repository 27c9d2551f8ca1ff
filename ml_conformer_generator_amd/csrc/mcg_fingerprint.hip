// Chemical fingerprints of molecular graphs ("Chemical fingerprints"): a circular, Morgan-type
// 2 048-bit fingerprint (radius 2, bond types on, chirality off) and a 64-bit graph identity key per molecule, and the
// Tanimoto of such fingerprints.  The package's OWN definition - a labelled substitute, NOT bit-compatible with RDKit's
// Morgan fingerprint.  H = MurmurHash3_x86_32 over uint32 words; integer arithmetic only, so every output is exact.
//   k_graph_fingerprint: one 64-lane workgroup (one wave) per molecule, lane = atom.  In LDS: the bond-code rows (68-byte
//                        stride: a lane walking its own row hits 32 different banks), the 64-bit neighbour masks, two
//                        invariant arrays, the 64 fingerprint words (LDS atomic OR) and the sorted invariants.
//                        ring(a): per neighbour j a level-by-level flood over the masks from a's other neighbours.
//                        Round r: the neighbours' (code, invariant) pairs go into the hash in ascending order, selected
//                        by repeated minimum passes over the neighbour mask (no per-lane array, no scratch).
//                        All K = max(n - 1, 2) rounds run in the launch (K is uniform in the workgroup); then the
//                        invariants are ranked by counting and two lanes hash the sorted sequence into the key.
//   k_fp_tanimoto:       16 lanes per molecule against one reference fingerprint.
//   k_fp_pair:           a 256-lane workgroup owns FP_ROWS rows x 256 columns of the matrix: a lane keeps its column's 64
//                        words in registers and walks the rows, whose words are uniform in the wave (scalar loads); row
//                        popcounts once per workgroup in LDS.  T = c / (p_i + p_j - c): c and p are exact integers and
//                        AND is commutative, so T is exactly symmetric and its diagonal exactly 1.
// An empty fingerprint (a molecule without atoms) has no similarity to anything: NaN, for its whole row and column.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_graph_rules.h"
#include "mcg_hash.h"
#include "mcg_ring_bonds.h"

namespace {

constexpr int FP_WORDS = MCG_FP_WORDS;       // 2 048 bits
constexpr int FP_MAXW = 64;                  // atoms per molecule: one lane each, one 64-bit neighbour mask each
constexpr int FP_ROWS = 64;                  // rows per workgroup of k_fp_pair
static_assert(FP_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");

__global__ __launch_bounds__(FP_MAXW) void k_graph_fingerprint(const int32_t* __restrict__ z,
                                                               const int8_t* __restrict__ bonds,
                                                               const int32_t* __restrict__ n_nodes, int W,
                                                               uint32_t* __restrict__ fp_out,
                                                               unsigned long long* __restrict__ key_out,
                                                               int32_t* __restrict__ pop_out) {
    __shared__ __attribute__((aligned(16))) uint8_t code[FP_MAXW * MCG_CODE_STRIDE];
    __shared__ unsigned long long nbr[FP_MAXW];
    __shared__ uint32_t inv[2][FP_MAXW];
    __shared__ uint32_t sorted[FP_MAXW];
    __shared__ uint32_t fpw[FP_WORDS];

    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), W);
    const bool real = a < n;

    // the molecule's W x W codes -> LDS rows; the diagonal, the padding and every code outside 1..4 become 0
    mcg_stage_codes(code, bonds + (size_t)b * W * W, W, n, a, FP_MAXW);
    fpw[a] = 0u;
    __syncthreads();

    const uint8_t* row = code + a * MCG_CODE_STRIDE;
    // its own row walk, not mcg_bond_tally: nothing here reads a by-code mask
    unsigned long long mine = 0ull;
    uint32_t deg = 0, val2 = 0;                  // val2: twice the bond-order sum, aromatic = 1.5
    if (real) {
        for (int j = 0; j < n; ++j) {
            const uint32_t c = row[j];
            if (c != 0) {
                mine |= 1ull << j;
                ++deg;
                val2 += c == 1 ? 2u : c == 2 ? 4u : c == 3 ? 6u : 3u;
            }
        }
    }
    nbr[a] = mine;
    __syncthreads();

    // ring(a): the smallest cycle through a (mcg_ring_bonds.h)
    const uint32_t ring = mcg_ring_bonds_of(nbr, a, mine, n).smallest;

    uint32_t cur = 0;
    if (real) {
        uint32_t h = MCG_HASH_SEED;
        h = mm3_mix(h, 0u);
        h = mm3_mix(h, (uint32_t)z[(size_t)b * W + a]);
        h = mm3_mix(h, deg);
        h = mm3_mix(h, val2);
        h = mm3_mix(h, ring);
        cur = mm3_final(h, 5u);
        atomicOr(&fpw[(cur & 2047u) >> 5], 1u << (cur & 31u));
    }
    inv[0][a] = cur;
    __syncthreads();

    const int K = max(n - 1, 2);
    for (int r = 1; r <= K; ++r) {
        const uint32_t* prev = inv[(r - 1) & 1];
        if (real) {
            uint32_t h = mm3_mix(mm3_mix(MCG_HASH_SEED, (uint32_t)r), cur);
            // ascending (code, invariant) pairs: each pass finds the smallest key above the last one and how often it occurs
            uint32_t emitted = 0;
            unsigned long long last = 0ull;          // real keys are >= 1 << 32 (code >= 1)
            while (emitted < deg) {
                unsigned long long best = ~0ull;
                uint32_t count = 0;
                for (unsigned long long f = mine; f != 0ull; f &= f - 1ull) {
                    const int j = low_bit(f);
                    const unsigned long long k = ((unsigned long long)row[j] << 32) | prev[j];
                    if (k > last) {
                        count = k < best ? 1u : count + (k == best ? 1u : 0u);
                        best = k < best ? k : best;
                    }
                }
                for (uint32_t t = 0; t < count; ++t) h = mm3_mix(mm3_mix(h, (uint32_t)(best >> 32)), (uint32_t)best);
                emitted += count;
                last = best;
            }
            cur = mm3_final(h, 2u + 2u * deg);
            if (r <= 2) atomicOr(&fpw[(cur & 2047u) >> 5], 1u << (cur & 31u));
        }
        inv[r & 1][a] = cur;
        __syncthreads();
    }

    // the key: the final invariants sorted ascending (rank by counting; equal values take consecutive ranks)
    const uint32_t* last_inv = inv[K & 1];
    if (real) {
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t v = last_inv[j];
            rank += (v < cur || (v == cur && j < a)) ? 1 : 0;
        }
        sorted[rank] = cur;
    }
    __syncthreads();
    uint32_t hk = 0;
    if (a < 2) {                                 // lane 0: the low half, lane 1: the high half
        hk = mm3_mix(a == 0 ? MCG_HASH_SEED : MCG_HASH_SEED_HI, (uint32_t)n);
        for (int j = 0; j < n; ++j) hk = mm3_mix(hk, sorted[j]);
        hk = mm3_final(hk, (uint32_t)n + 1u);
    }
    const uint32_t key_hi = __shfl(hk, 1);
    if (a == 0) key_out[b] = ((unsigned long long)key_hi << 32) | hk;
    const uint32_t word = fpw[a];
    fp_out[(size_t)b * FP_WORDS + a] = word;
    if (pop_out != nullptr) {
        const int p = wave_sum(__popc(word));
        if (a == 0) pop_out[b] = p;
    }
}

__device__ __forceinline__ float tanimoto_of(int c, int pa, int pb) {
    if (pa == 0 || pb == 0) return __builtin_nanf("");
    return (float)c / (float)(pa + pb - c);
}

__global__ __launch_bounds__(256) void k_fp_tanimoto(const uint32_t* __restrict__ fp, const uint32_t* __restrict__ ref,
                                                     int B, float* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long b = t >> 4;
    const int q = (int)(t & 15);
    int c = 0, pa = 0, pb = 0;
    if (b < B) {
        const uint4 x = reinterpret_cast<const uint4*>(fp + (size_t)b * FP_WORDS)[q];
        const uint4 y = reinterpret_cast<const uint4*>(ref)[q];
        c = __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
        pa = __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
        pb = __popc(y.x) + __popc(y.y) + __popc(y.z) + __popc(y.w);
    }
    for (int off = 8; off > 0; off >>= 1) {
        c += __shfl_xor(c, off);
        pa += __shfl_xor(pa, off);
        pb += __shfl_xor(pb, off);
    }
    if (b < B && q == 0) out[b] = tanimoto_of(c, pa, pb);
}

__global__ __launch_bounds__(256) void k_fp_pair(const uint32_t* __restrict__ fp, int B, float* __restrict__ out) {
    __shared__ int row_pop[FP_ROWS];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * FP_ROWS;
    const int rows = min(FP_ROWS, B - i0);
    const long j = (long)blockIdx.x * 256 + tid;
    if (tid < rows) {
        const uint4* r = reinterpret_cast<const uint4*>(fp + (size_t)(i0 + tid) * FP_WORDS);
        int p = 0;
        for (int q = 0; q < FP_WORDS / 4; ++q) {
            const uint4 v = r[q];
            p += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        }
        row_pop[tid] = p;
    }
    uint32_t col[FP_WORDS];
    int pj = 0;
    {
        const uint4* cptr = reinterpret_cast<const uint4*>(fp + (size_t)(j < B ? j : 0) * FP_WORDS);
#pragma unroll
        for (int q = 0; q < FP_WORDS / 4; ++q) {
            const uint4 v = cptr[q];
            col[4 * q] = v.x, col[4 * q + 1] = v.y, col[4 * q + 2] = v.z, col[4 * q + 3] = v.w;
            pj += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        }
    }
    __syncthreads();
    if (j >= B) return;
    float* dst = out + (size_t)i0 * B + j;
#pragma unroll 1
    for (int r = 0; r < rows; ++r) {
        const uint32_t* arow = fp + (size_t)(i0 + r) * FP_WORDS;      // uniform in the workgroup: scalar loads
        int c = 0;
#pragma unroll
        for (int w = 0; w < FP_WORDS; ++w) c += __popc(arow[w] & col[w]);
        dst[(size_t)r * B] = tanimoto_of(c, row_pop[r], pj);
    }
}

}  // namespace

extern "C" int mcg_graph_fingerprint(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                                     uint32_t* fp_out, uint64_t* key_out, int32_t* popcount_out, void* stream) {
    if (!z || !bonds || !n_nodes_dev || !fp_out || !key_out || B < 0 || W < 1 || W > FP_MAXW) {
        mcg_set_error("mcg_graph_fingerprint: bad arguments (non-null z, bonds, n_nodes, fp_out and key_out, B >= 0, "
                      "1 <= W <= %d)", FP_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_graph_fingerprint, dim3((unsigned)B), dim3(FP_MAXW), 0, (hipStream_t)stream, z, bonds,
                       n_nodes_dev, W, fp_out, reinterpret_cast<unsigned long long*>(key_out), popcount_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_fingerprint_tanimoto(const uint32_t* fp, const uint32_t* ref_fp, int B, float* out, void* stream) {
    if (!fp || !ref_fp || !out || B < 0) {
        mcg_set_error("mcg_fingerprint_tanimoto: bad arguments (non-null fp, ref_fp and out, B >= 0)");
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_fp_tanimoto, dim3((unsigned)(((long)B * 16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fp,
                       ref_fp, B, out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_fingerprint_pair_tanimoto(const uint32_t* fp, int B, float* out, void* stream) {
    if (!fp || !out || B < 0 || B > MCG_SHAPE_PAIR_MAX_B) {
        mcg_set_error("mcg_fingerprint_pair_tanimoto: bad arguments (non-null fp and out, 0 <= B <= %d)",
                      MCG_SHAPE_PAIR_MAX_B);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_fp_pair, dim3((unsigned)((B + 255) / 256), (unsigned)((B + FP_ROWS - 1) / FP_ROWS)), dim3(256), 0,
                       (hipStream_t)stream, fp, B, out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
