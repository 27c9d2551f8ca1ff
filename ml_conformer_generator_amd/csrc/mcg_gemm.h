// Node-side GEMMs of the EGNN and the Linear layers of the GCN: argument blocks, weight packers and the launchers of
// mcg_gemm.hip (kernel templates: mcg_gemm_kernels.h).
//     C[M, n_out] = epilogue( [A1 | A2][M, K1+K2] * B + bias ) (+ residual)
//
// "B-pack4" layout of a weight W[n_out][K] (nn.Linear layout), per K segment:
//   full 16-k groups:  Bp4[((q * n_tiles + nt) * 64 + lane) * 4 + s] = W[16 nt + (lane&15)][16 q + 4 (lane>>4) + s]
//   then tail steps:   Bp4[tail_base + (st * n_tiles + nt) * 64 + lane] = W[16 nt + (lane&15)][16 Q + 4 st + (lane>>4)]
// i.e. one 16-byte load gives a lane its B operand for the 4 k-steps of a group, matching
// the 16-byte load of 4 consecutive k of its A row (k permutation: mcg_common.h).
#pragma once
#include "mcg_common.h"
#include "../../include/mlconfgen_hip.h"

#include <vector>

enum { MCG_ACT_NONE = 0, MCG_ACT_SILU = 1, MCG_ACT_RELU = 2 };

struct McgGemmArgs {
    const float* A1; int lda1; int K1;      // first K segment  (K1 % 4 == 0)
    const float* A2; int lda2; int K2;      // optional second segment (concat along K), K2 may be 0
    const float* Bp;                        // B-pack4 of segment 1 followed by B-pack4 of segment 2
    const float* bias;                      // [n_tiles*16] (padded) or nullptr
    const float* resid; int ldr;            // optional residual added after activation; ONLY with n_store % 4 == 0: the kernels load it in
                                            // 16-byte pieces and a ragged last piece would lose it (the launchers refuse the combination)
    float* C; int ldc;
    int M; int n_tiles; int n_store;        // columns >= n_store are not written
    int act;
    // --- gathering kernels only (value-initialise the struct: zero = unused) ---
    const int4* a2_rows;                    // optional: row r of segment 2 is the SUM of the first a2_nsum (2..4) of rows
    int a2_nsum;                            // a2_rows[r].x .y .z .w of A2: the workgroup-level partial-sum slots of an atom (mcg_plan_host.cpp)
    // side job run by the blocks beyond the GEMM's own grid (independent data, saves a launch):
    // x[v][0..2] += (side_u[s.x] + side_u[s.y] + side_u[s.z] + side_u[s.w]) / 100 - the coordinate update of the previous block (egnn.py:128-148)
    const float* side_u; const int4* side_slots; float* side_x; int side_M;
    int gemm_blocks;                        // workgroups of the GEMM proper (set by the launcher)
    // mcg_gemm_launch and mcg_gemm_bf16_launch only (the 16-row and split-operand launchers refuse it), and only with n_tiles == 54
    // (two parts of 27 column tiles): C is the BLOCKED layer-1 input layout of the bf16 edge kernel, C[part][k-block][piece][row][4] with
    // column = part * 432 + 32 * k-block + 4 * piece + (0..3): a 16-byte piece of 16 consecutive rows is 256 contiguous bytes,
    // so the 16 rows (i, j .. j+15) of an edge tile read their gathered half with ADJACENT LANES ON ADJACENT ADDRESSES
    // (mcg_edge_bf16.hip, BLK; tools/native/gather_probe.hip: 88 ns instead of 224 per instruction and wave)
    int c_blocked;
};

// floats occupied by one K segment of a B-pack4
__host__ __device__ static inline size_t mcg_pack4_floats(int K, int n_tiles) { return (size_t)(K / 4) * n_tiles * 64; }

template <class F>
static void mcg_pack_b4(std::vector<float>& dst, int K, int n_tiles, F value /* (n, k) -> W[n][k] or 0 */) {
    const size_t base = dst.size();
    dst.resize(base + mcg_pack4_floats(K, n_tiles), 0.f);
    const int groups = K / 16, tail = (K - groups * 16) / 4;
    float* d = dst.data() + base;
    for (int q = 0; q < groups; ++q)
        for (int nt = 0; nt < n_tiles; ++nt)
            for (int l = 0; l < 64; ++l)
                for (int s = 0; s < 4; ++s)
                    d[(((size_t)q * n_tiles + nt) * 64 + l) * 4 + s] = value(nt * 16 + (l & 15), 16 * q + 4 * (l >> 4) + s);
    float* t = d + (size_t)groups * n_tiles * 256;
    for (int st = 0; st < tail; ++st)
        for (int nt = 0; nt < n_tiles; ++nt)
            for (int l = 0; l < 64; ++l)
                t[((size_t)st * n_tiles + nt) * 64 + l] = value(nt * 16 + (l & 15), 16 * groups + 4 * st + (l >> 4));
}

// ---------------------------------------------------------------------------------------------
// bf16-operand variant (fp32 accumulate, fp32 in/out): v_mfma_f32_16x16x32_bf16.  K is consumed in
// blocks of 32 (K padded up with ZERO weights; the activation rows are read past K into finite
// padding/neighbouring data that the zero weights cancel).  "B-pack16" layout per K segment:
//   Bp16[((kb * n_tiles + nt) * 64 + lane) * 8 + j] = bf16( W[16 nt + (lane&15)][32 kb + 8 (lane>>4) + j] )
// A rows are loaded as fp32 (two 16-byte loads per k-block) and rounded to bf16 in registers.
__host__ __device__ static inline int mcg_kblocks16(int K) { return (K + 31) / 32; }
__host__ __device__ static inline size_t mcg_pack16_elems(int K, int n_tiles) { return (size_t)mcg_kblocks16(K) * n_tiles * 64 * 8; }

template <class F>
static void mcg_pack_b16(std::vector<uint16_t>& dst, int K, int n_tiles, F value /* (n, k) -> W[n][k] or 0 */) {
    const size_t base = dst.size();
    dst.resize(base + mcg_pack16_elems(K, n_tiles), 0);
    uint16_t* d = dst.data() + base;
    for (int kb = 0; kb < mcg_kblocks16(K); ++kb)
        for (int nt = 0; nt < n_tiles; ++nt)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 32 * kb + 8 * (l >> 4) + j;
                    d[(((size_t)kb * n_tiles + nt) * 64 + l) * 8 + j] = k < K ? mcg_f32_to_bf16_bits(value(nt * 16 + (l & 15), k)) : 0;
                }
}

// "B-pack16x3" (f32x6 GEMM): every weight as the exact sum of three bf16 parts, [k-block][part][n-tile][lane][8]
template <class F>
static void mcg_pack_b16x3(std::vector<uint16_t>& dst, int K, int n_tiles, F value /* (n, k) -> W[n][k] or 0 */) {
    const size_t base = dst.size();
    const int kbn = mcg_kblocks16(K);
    dst.resize(base + (size_t)kbn * 3 * n_tiles * 64 * 8, 0);
    uint16_t* d = dst.data() + base;
    for (int kb = 0; kb < kbn; ++kb)
        for (int nt = 0; nt < n_tiles; ++nt)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 32 * kb + 8 * (l >> 4) + j;
                    float r = k < K ? value(nt * 16 + (l & 15), k) : 0.f;
                    for (int part = 0; part < 3; ++part) {
                        const uint16_t hb = mcg_f32_to_bf16_bits(r);
                        d[((((size_t)kb * 3 + part) * n_tiles + nt) * 64 + l) * 8 + j] = hb;
                        uint32_t u = (uint32_t)hb << 16;
                        float f;
                        __builtin_memcpy(&f, &u, 4);
                        r -= f;
                    }
                }
}
__host__ __device__ static inline size_t mcg_pack16x3_elems(int K, int n_tiles) { return 3 * mcg_pack16_elems(K, n_tiles); }

// bf16 mode, large batches: the node phase of ONE GCL layer in one launch (W3 + gather, W4 + residual, the next edge layer's
// first-layer projections; mcg_gemm.hip)
struct McgNodeFusedArgs {
    const float* h; int ldh;                    // [M][ldh] fp32, K = 420 real columns
    const float* P; int ldp;                    // per-unit partial sums (NOT divided by 100) or a materialised aggregate
    const int4* a2_rows; int a2_nsum;           // the atom's partial rows (GATHER 2 / 4)
    const uint16_t* w3; const float* b3;        // B-pack16 of W3: [28 k-blocks][27 tiles][64][8]
    const uint16_t* w4; const float* b4;        // [14][27][64][8]
    float* h_out; int ldo;                      // h' (fp32)
    const uint16_t* wab; const float* bab;      // next layer's first edge layer: [14][54][64][8], bias [864] (b1 | 0)
    float* pab; int ldpab; int pab_blocked;     // Pab' in the edge kernel's layout
    int M;
};
constexpr int MCG_NF_MIN_ROWBLOCKS = 32;        // automatic choice of the fused node launch: from 32 row blocks (1 024 atoms) on

// The template instantiation a launcher dispatched: the kernel and its template arguments (0 where the template has none).
struct McgGemmRan { int kernel /* MCG_GEMM_KERNEL_* (mlconfgen_hip.h) */, rn, mr, ring, gather, resid, seg2; };
const McgGemmRan& mcg_gemm_last_launch();      // of the calling thread (mcg_debug_gemm)

// What no kernel implements and every launcher refuses: a residual on a ragged right edge (n_store % 4 != 0), and the blocked C
// layout outside the kernels that store through mcg_gemm_c_ptr (`blocked_ok`: mcg_gemm_launch, mcg_gemm_bf16_launch) or with
// another width than its 2 x 27 column tiles.
bool mcg_gemm_out_of_contract(const McgGemmArgs& a, bool blocked_ok);

// Launchers (each returns hipGetLastError(); M <= 0 launches nothing; hipErrorInvalidValue, nothing launched, for a residual with
// n_store % 4 != 0 and for c_blocked where it is not implemented).  `rn_override` 1..3 fixes the wave tile width
// (MCG_OPT_GEMM_RN / MCG_OPT_GEMM_X6_RN), 0 = the launcher's cost model.  A launcher whose kernel carries the coordinate-update
// side job (side_x set) adds its workgroups behind the GEMM's own.
hipError_t mcg_gemm_launch(McgGemmArgs a, int rn_override, hipStream_t s);               // fp32, 32-row wave tiles
hipError_t mcg_gemm16_launch(McgGemmArgs a, int rn, int mr, bool deep, hipStream_t s);   // fp32, 16-row wave tiles
// bf16 operands: the 32-row kernel, or the LDS-staged 9-wave kernel (`lds` = MCG_OPT_GEMM_BF16_LDS: 0 automatic, 1 never,
// 2 whenever its shape limits allow)
hipError_t mcg_gemm_bf16_launch(McgGemmArgs a, int rn_override, int lds, hipStream_t s);
hipError_t mcg_gemm_x6_launch(const McgGemmArgs& a, int rn_override, hipStream_t s);     // f32x6: Bp is a B-pack16x3, no side job
hipError_t mcg_node_fused_launch(const McgNodeFusedArgs& a, hipStream_t s);
