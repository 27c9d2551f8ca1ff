// Kernel templates of the node / GCN GEMMs, included by mcg_gemm.hip (and the measurement tool tools/native/gemm_bench.hip).
// The fp32 kernels run on v_mfma_f32_16x16x4_f32: a 256-thread workgroup owns 32 rows x (4 waves x RN column tiles); each
// wave keeps a 2 x RN grid of 16x16 accumulators.  Operands come straight from global memory with 16-byte loads, register
// double-buffered one 16-k group ahead of the MFMAs: the four waves of a workgroup read the SAME 32 A rows (shared through
// the CU's L1) and disjoint packed-B columns.  No LDS, no barriers.
#pragma once
#include "mcg_gemm.h"

#include <type_traits>

// Workgroups are numbered through mcg_xcd_remap, an XCD-aware order: block b runs on XCD b % 8 (observed; speed only).  With
// the linear (row block, wave column) numbering a contiguous block range is a band of rows x all columns, so after the remap
// every XCD reads 1/8 of A and all of B into its L2 instead of nearly all of both (config 2 Pab GEMM: 35 MB -> 14.5 MB of
// fabric traffic per launch).

// address of C[row][16 * nt + 4 * g .. + 3] (nt = column tile): row-major, or the blocked layout above (27 column tiles per part,
// 14 k-blocks of two tiles = eight 4-column pieces each; the upper four pieces of the 14th block stay zero)
__device__ __forceinline__ float* mcg_gemm_c_ptr(const McgGemmArgs& p, int orow, int nt, int g) {
    if (!p.c_blocked) return p.C + (size_t)orow * p.ldc + nt * 16 + 4 * g;
    const int part = nt >= 27 ? 1 : 0, ntp = nt - 27 * part;
    return p.C + ((size_t)((part * 14 + (ntp >> 1)) * 8 + (ntp & 1) * 4 + g) * p.M + orow) * 4;
}

// Side job of the fp32 node GEMM launches (workgroups beyond the GEMM's own grid): the coordinate update of the
// previous EquivariantBlock, x[v] += (u[s.x] + u[s.y] + u[s.z] + u[s.w]) / 100 (egnn.py:128-148) - independent data, saves a launch.
__device__ __forceinline__ void mcg_gemm_side_job(const McgGemmArgs& p, int block) {
    const int idx = block * 256 + (int)threadIdx.x;
    const int v = idx >> 2, comp = idx & 3;
    if (v < p.side_M && comp < 3) {
        const int4 sl = p.side_slots[v];
        p.side_x[(size_t)v * 4 + comp] += (((p.side_u[(size_t)sl.x * 4 + comp] + p.side_u[(size_t)sl.y * 4 + comp]) + p.side_u[(size_t)sl.z * 4 + comp]) +
                                           p.side_u[(size_t)sl.w * 4 + comp]) / 100.0f;
    }
}

// GATHER (0 / 2 / 4): row r of the SECOND K segment is (A2[s.x] + A2[s.y] (+ A2[s.z] + A2[s.w])) / 100 with s = a2_rows[r] -
// the per-unit partial sums of the 64-row edge kernel (one row per unit and atom, NOT yet divided by 100; unused slots
// name the common zero row), i.e. the aggregate of egnn.py:59-64,435 read straight from the edge kernel's output: no
// combine launch.  Workgroups beyond `gemm_blocks` run the coordinate-update side job like the fp32 kernels.
template <int RN, int GATHER = 0>
__global__ __launch_bounds__(256) void mcg_gemm_bf16_kernel(McgGemmArgs p) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int wave_cols = (p.n_tiles + RN - 1) / RN;
    const int nblk = p.gemm_blocks > 0 ? p.gemm_blocks : (int)gridDim.x;        // (+ side-job workgroups behind them)
    if ((int)blockIdx.x >= nblk) { mcg_gemm_side_job(p, (int)blockIdx.x - nblk); return; }
    const int wlin = mcg_xcd_remap(blockIdx.x, nblk) * 4 + wid;
    if (wlin >= ((p.M + 31) / 32) * wave_cols) return;
    const int row0 = (wlin / wave_cols) * 32;
    const int nt0 = (wlin % wave_cols) * RN;
    int rA[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int r = row0 + 16 * m + c;
        rA[m] = r < p.M ? r : p.M - 1;
    }
    bool nvalid[RN];
    int ncl[RN];
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        nvalid[n] = nt0 + n < p.n_tiles;
        ncl[n] = nvalid[n] ? n : 0;
    }
    f32x4 acc[2][RN];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < RN; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // Accumulators are kept TRANSPOSED (weights as the MFMA A operand, activations as B: the two operands have
    // the same lane layout, so this is just the argument order): lane (c, g) of tile (m, n) then holds output
    // row row0 + 16m + c, columns 16(nt0+n) + 4g .. +3 - four consecutive floats, so bias, residual and the
    // result move as 16-byte vectors (6 stores per wave tile instead of 24 dword stores).
    // Epilogue operands are fetched NOW so their latency hides under the K loop.
    f32x4 ebias[RN];
    f32x4 eres[2][RN];
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        const int col = (nt0 + ncl[n]) * 16 + 4 * g;
        ebias[n] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int orow = row0 + 16 * m + c;
            eres[m][n] = (p.resid && orow < p.M && col + 3 < p.n_store) ? *reinterpret_cast<const f32x4*>(p.resid + (size_t)orow * p.ldr + col)
                                                                        : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }

    const bf16x8* bseg = reinterpret_cast<const bf16x8*>(p.Bp);
    auto ld = [](const __amdgpu_buffer_rsrc_t& r, unsigned v, int so) { return __builtin_amdgcn_raw_buffer_load_b128(r, (int)v, so, 0); };
    // one K segment whose row r of A is the sum of NS rows (NS = 1: the row itself) scaled by `scale_div100`
    auto segment = [&](auto ns_tag, const float* A, int K, int lda, const int (&ra)[2][4]) {
        constexpr int NS = decltype(ns_tag)::value;
        const int blocks = mcg_kblocks16(K);
        const size_t bstride = (size_t)p.n_tiles * 64;        // bf16x8 elements per k-block
        // 3-deep register ring, same discipline as the fp32 kernel (pinned order, unconditional loads)
        f32x4 Ar[3][2][NS][2];
        bf16x8 Br[3][RN];
        const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A), 0, 0xffffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8*>(bseg), 0, 0xffffffff, 0x00020000);
        unsigned oa[2][NS];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int q = 0; q < NS; ++q) oa[m][q] = (unsigned)(ra[m][q] * lda + 8 * g) * 4u;
        unsigned obn[RN];
#pragma unroll
        for (int n = 0; n < RN; ++n) obn[n] = (unsigned)((nt0 + ncl[n]) * 64 + lane) * 16u;
        const int bbytes = p.n_tiles * 64 * 16;
        auto load_block = [&](int slot, int kb) {
            kb = kb < blocks ? kb : blocks - 1;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    Ar[slot][m][q][0] = __builtin_bit_cast(f32x4, ld(rs_a, oa[m][q], 128 * kb));
                    Ar[slot][m][q][1] = __builtin_bit_cast(f32x4, ld(rs_a, oa[m][q], 128 * kb + 16));
                }
#pragma unroll
            for (int n = 0; n < RN; ++n) Br[slot][n] = __builtin_bit_cast(bf16x8, ld(rs_b, obn[n], kb * bbytes));
        };
        auto row_value = [&](int slot, int m, int half) -> f32x4 {
            f32x4 v = Ar[slot][m][0][half];
            if constexpr (NS > 1) {
#pragma unroll
                for (int q = 1; q < NS; ++q) v += Ar[slot][m][q][half];     // slot order = unit order: fixed, deterministic
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = mcg_div100(v[r]);       // the aggregate's / normalization_factor (egnn.py:435)
            }
            return v;
        };
        auto compute = [&](int slot) {
            const bf16x8 A0 = mcg_pack_bf16(row_value(slot, 0, 0), row_value(slot, 0, 1));
            const bf16x8 A1 = mcg_pack_bf16(row_value(slot, 1, 0), row_value(slot, 1, 1));
#pragma unroll
            for (int n = 0; n < RN; ++n) {
                acc[0][n] = mcg_mfma_bf16(Br[slot][n], A0, acc[0][n]);
                acc[1][n] = mcg_mfma_bf16(Br[slot][n], A1, acc[1][n]);
            }
        };
        load_block(0, 0); load_block(1, 1); load_block(2, 2);
        int kb = 0;
#pragma unroll 1
        for (; kb + 3 <= blocks; kb += 3) {
            compute(0); __builtin_amdgcn_sched_barrier(0); load_block(0, kb + 3); __builtin_amdgcn_sched_barrier(0);
            compute(1); __builtin_amdgcn_sched_barrier(0); load_block(1, kb + 4); __builtin_amdgcn_sched_barrier(0);
            compute(2); __builtin_amdgcn_sched_barrier(0); load_block(2, kb + 5); __builtin_amdgcn_sched_barrier(0);
        }
        if (kb < blocks) compute(0);
        if (kb + 1 < blocks) compute(1);
        bseg += (size_t)blocks * bstride;
    };
    int ra[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) ra[m][q] = rA[m];
    if (p.K1 > 0) segment(std::integral_constant<int, 1>{}, p.A1, p.K1, p.lda1, ra);
    if (p.K2 > 0) {
        if constexpr (GATHER >= 2) {
#pragma unroll
            for (int m = 0; m < 2; ++m) { const int4 sl = p.a2_rows[rA[m]]; ra[m][0] = sl.x; ra[m][1] = sl.y; ra[m][2] = sl.z; ra[m][3] = sl.w; }
            segment(std::integral_constant<int, GATHER>{}, p.A2, p.K2, p.lda2, ra);
        } else {
            segment(std::integral_constant<int, 1>{}, p.A2, p.K2, p.lda2, ra);
        }
    }
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        if (!nvalid[n]) continue;
        const int col = (nt0 + n) * 16 + 4 * g;
        if (col >= p.n_store) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int orow = row0 + 16 * m + c;
            if (orow >= p.M) continue;
            f32x4 v = acc[m][n] + ebias[n];
            if (p.act == MCG_ACT_SILU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = mcg_silu(v[r]);
            } else if (p.act == MCG_ACT_RELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            v += eres[m][n];
            float* dst = mcg_gemm_c_ptr(p, orow, nt0 + n, g);
            if (col + 3 < p.n_store) {
                *reinterpret_cast<f32x4*>(dst) = v;       // (4-byte aligned is enough for a global dwordx4 store)
            } else {                                       // ragged right edge (GCN: 210 columns)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col + r < p.n_store) dst[r] = v[r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// bf16 node GEMM for LARGE batches (round 5): the activation block of a workgroup goes through LDS ONCE.
// PMC of the kernel above at 6 895 rows (profiles/round5_c3_bf16_pmc_stall.csv): 67 % of its wave-cycles wait to ISSUE
// (SQ_WAIT_INST_ANY) with the matrix pipe 5 % busy - every wave loads its own copy of the 32 activation rows (9 column
// groups re-read each row block: 364 MB through the vector L1s per launch for 23 MB of activations) and the texture
// addresser is the bottleneck.  Here a workgroup owns 32 rows x 27 column tiles (ALL columns of a 432-wide output; the
// 864-wide first-layer GEMM takes two workgroups per row block): its 9 waves load the fp32 block cooperatively, sum the
// gathered partial rows, divide by 100, round to bf16 and park the result in LDS as ready-made MFMA fragments
// ([k-block][row tile][lane] x 16 B: a wave's ds_read_b128 is 1 KB contiguous, conflict-free) - ONE barrier, after which
// each wave walks K alone: two fragment reads + its three weight fragments (a 4-deep register ring straight from L2;
// weights are per-wave disjoint, there is nothing to share) + six MFMAs per 32-k block.  Same operand values, same k order
// per output element as the kernel above: bit-identical results (tests/test_hip_parity.py).
constexpr int MCG_LDSG_WAVES = 9, MCG_LDSG_RN = 3, MCG_LDSG_THREADS = MCG_LDSG_WAVES * 64, MCG_LDSG_TILES = MCG_LDSG_WAVES * MCG_LDSG_RN;
constexpr int MCG_LDSG_MAX_BLOCKS = 28;                 // k-blocks of 32 a workgroup can park: 28 x 2 KB = 56 KB of LDS
constexpr int MCG_LDSG_S2P = 2;                         // k-blocks of the SECOND K segment one wave parks (b2 <= S2P x WAVES)

__device__ __forceinline__ void mcg_gemm_side_job_n(const McgGemmArgs& p, int block, int threads) {
    const int idx = block * threads + (int)threadIdx.x;
    const int v = idx >> 2, comp = idx & 3;
    if (v < p.side_M && comp < 3) {
        const int4 sl = p.side_slots[v];
        p.side_x[(size_t)v * 4 + comp] += (((p.side_u[(size_t)sl.x * 4 + comp] + p.side_u[(size_t)sl.y * 4 + comp]) + p.side_u[(size_t)sl.z * 4 + comp]) +
                                           p.side_u[(size_t)sl.w * 4 + comp]) / 100.0f;
    }
}

template <int GATHER, bool RESID, bool SEG2, int RING>
__global__ __launch_bounds__(MCG_LDSG_THREADS) void mcg_gemm_bf16_lds_kernel(McgGemmArgs p) {
    __shared__ bf16x8 sA[MCG_LDSG_MAX_BLOCKS * 2 * 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int nblk = p.gemm_blocks > 0 ? p.gemm_blocks : (int)gridDim.x;        // (+ side-job workgroups behind them)
    if ((int)blockIdx.x >= nblk) { mcg_gemm_side_job_n(p, (int)blockIdx.x - nblk, MCG_LDSG_THREADS); return; }
    const int col_groups = (p.n_tiles + MCG_LDSG_TILES - 1) / MCG_LDSG_TILES;
    const int wg = mcg_xcd_remap(blockIdx.x, nblk);
    const int row0 = (wg / col_groups) * 32;
    const int nt0 = (wg % col_groups) * MCG_LDSG_TILES + wid * MCG_LDSG_RN;
    constexpr int RN = MCG_LDSG_RN;
    bool nvalid[RN];
    int ncl[RN];
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        nvalid[n] = nt0 + n < p.n_tiles;
        ncl[n] = nvalid[n] ? nt0 + n : 0;
    }
    const int b1 = p.K1 > 0 ? mcg_kblocks16(p.K1) : 0, b2 = (SEG2 && p.K2 > 0) ? mcg_kblocks16(p.K2) : 0;
    const int blocks = b1 + b2;

    // ---- the weight ring starts first: its loads fly while the activation block is being parked
    const bf16x8* bseg = reinterpret_cast<const bf16x8*>(p.Bp);
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8*>(bseg), 0, 0xffffffff, 0x00020000);
    auto ld = [](const __amdgpu_buffer_rsrc_t& r, unsigned v, int so) { return __builtin_amdgcn_raw_buffer_load_b128(r, (int)v, so, 0); };
    unsigned obn[RN];
#pragma unroll
    for (int n = 0; n < RN; ++n) obn[n] = (unsigned)(ncl[n] * 64 + lane) * 16u;
    const int bbytes = p.n_tiles * 64 * 16;                  // bytes per k-block of the pack (both segments: same n_tiles, contiguous)
    bf16x8 Br[RING][RN];
    auto load_w = [&](int slot, int kb) {
        kb = kb < blocks ? kb : blocks - 1;
#pragma unroll
        for (int n = 0; n < RN; ++n) Br[slot][n] = __builtin_bit_cast(bf16x8, ld(rs_b, obn[n], kb * bbytes));
    };
#pragma unroll
    for (int r = 0; r < RING; ++r) load_w(r, r);

    int rr[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int r = row0 + 16 * m + c; rr[m] = r < p.M ? r : p.M - 1; }

    // ---- park the activation block.  LOADS ARE COALESCED, the MFMA layout is made on the way into LDS: read the way the
    //      fragments want it (lane 16 g + c = row c, slice g) adjacent lanes sit in different rows and an instruction costs the
    //      memory pipeline 224 ns per wave instead of 88 (tools/native/gather_probe.hip).  So lane l of a load takes the 16-byte
    //      piece l % 8 of row 8 i + l / 8 (i = 0..3: a quarter of the 32 rows; 8 whole 128-byte lines per instruction), rounds its
    //      four values to bf16 and writes those 8 bytes where lane 16 (piece / 2) + row % 16 of fragment (k-block, row / 16) will
    //      read its ds_read_b128.  A wave owns the k-blocks wid, wid + 9 of each segment.
    const int prow = lane >> 3, piece = lane & 7;
    int qrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int r = row0 + 8 * i + prow; qrow[i] = r < p.M ? r : p.M - 1; }
    auto park_quarter = [&](int frag_kb, int i, f32x4 v, int k0, int K) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e >= K) v[e] = 0.f;                            // k beyond the segment: zero (the packed weights are zero there too)
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        const bf16x4 h4 = (bf16x4){(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        char* dst = reinterpret_cast<char*>(sA) + (((2 * frag_kb + (i >> 1)) * 64 + 16 * (piece >> 1) + 8 * (i & 1) + prow) * 16 + (piece & 1) * 8);
        *reinterpret_cast<bf16x4*>(dst) = h4;
    };
    {
        const __amdgpu_buffer_rsrc_t rs_a1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A1), 0, 0xffffffff, 0x00020000);
        for (int kb = wid; kb < b1; kb += MCG_LDSG_WAVES) {
            f32x4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = __builtin_bit_cast(f32x4, ld(rs_a1, (unsigned)(qrow[i] * p.lda1 + 32 * kb + 4 * piece) * 4u, 0));
#pragma unroll
            for (int i = 0; i < 4; ++i) park_quarter(kb, i, v[i], 32 * kb + 4 * piece, p.K1);
        }
    }
    // ---- segment 2: plain rows, or the sum of an atom's <= GATHER partial rows / 100 (slot order, then mcg_div100, then the
    //      bf16 rounding - exactly the A-loader of mcg_gemm_bf16_kernel).  Its loads are ISSUED here, in front of the first
    //      barrier, and consumed behind the K loop over segment 1 (their latency hides under it)
    constexpr int NS = GATHER >= 2 ? GATHER : 1;
    constexpr int S2P = SEG2 ? MCG_LDSG_S2P : 0;           // k-blocks of segment 2 per wave (b2 <= 18 = S2P x 9 waves: mcg_gemm_bf16_lds_ok)
    f32x4 s2[SEG2 ? 2 : 1][4][NS];
    const __amdgpu_buffer_rsrc_t rs_a2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A2 ? p.A2 : p.A1), 0, 0xffffffff, 0x00020000);
    int srow[4][NS];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (GATHER >= 2) {
            const int4 sl = (SEG2 && p.a2_rows) ? p.a2_rows[qrow[i]] : (int4){0, 0, 0, 0};
            const int rows[4] = {sl.x, sl.y, sl.z, sl.w};
#pragma unroll
            for (int q = 0; q < NS; ++q) srow[i][q] = rows[q];
        } else {
            srow[i][0] = qrow[i];
        }
    }
    auto seg2_issue = [&](int j) {
        int kb = wid + j * MCG_LDSG_WAVES;
        kb = kb < b2 ? kb : b2 - 1;                                     // (clamped: unconditional loads, the park is predicated)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < NS; ++q)
                s2[j][i][q] = __builtin_bit_cast(f32x4, ld(rs_a2, (unsigned)(srow[i][q] * p.lda2 + 32 * kb + 4 * piece) * 4u, 0));
    };
    auto seg2_park = [&](int j) {
        const int kb = wid + j * MCG_LDSG_WAVES;
        if (kb >= b2) return;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 v = s2[j][i][0];
            if constexpr (GATHER >= 2) {
#pragma unroll
                for (int q = 1; q < NS; ++q) v += s2[j][i][q];          // slot order = unit order: fixed, deterministic
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = mcg_div100(v[e]);   // the aggregate's / normalization_factor (egnn.py:435)
            }
            park_quarter(b1 + kb, i, v, 32 * kb + 4 * piece, p.K2);
        }
    };
    // the residual rows (W4: h) are requested here, a whole K loop ahead of their use
    f32x4 eres[RESID ? 2 : 1][RN];
    if constexpr (RESID) {
#pragma unroll
        for (int n = 0; n < RN; ++n) {
            const int col = ncl[n] * 16 + 4 * g;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int orow = row0 + 16 * m + c;
                eres[m][n] = (orow < p.M && col + 3 < p.n_store) ? *reinterpret_cast<const f32x4*>(p.resid + (size_t)orow * p.ldr + col)
                                                                  : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    constexpr bool OVERLAP2 = SEG2 && GATHER <= 2;  // (4-row gathers would hold 128 registers across the loop: park them up front)
    if (SEG2 && b2 > 0) {
        if constexpr (OVERLAP2) {
#pragma unroll
            for (int j = 0; j < S2P; ++j) seg2_issue(j);
        } else {
#pragma unroll
            for (int j = 0; j < S2P; ++j) { seg2_issue(j); seg2_park(j); }
        }
    }
    // (not __syncthreads(): hipcc drains the vector-memory counter in front of it, which would wait out the weight ring, the
    //  residual rows and the second segment's loads - exactly what is meant to stay in flight across this rendezvous)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ---- K loop: barrier-free, one wave = 2 x RN accumulators (transposed: weights as the MFMA A operand, see above)
    f32x4 acc[2][RN];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < RN; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int slot, int kb) {
        const bf16x8 A0 = sA[(2 * kb) * 64 + lane];
        const bf16x8 A1 = sA[(2 * kb + 1) * 64 + lane];
#pragma unroll
        for (int n = 0; n < RN; ++n) {
            acc[0][n] = mcg_mfma_bf16(Br[slot][n], A0, acc[0][n]);
            acc[1][n] = mcg_mfma_bf16(Br[slot][n], A1, acc[1][n]);
        }
    };
    // blocks [k0, k1) with the ring freshly loaded with k0, k0 + 1, k0 + 2 (every slot index is a compile-time constant:
    // a runtime slot would turn the ring into a scratch array)
    auto k_loop = [&](int k0, int k1) {
        int kb = k0;
#pragma unroll 1
        for (; kb + RING <= k1; kb += RING) {
#pragma unroll
            for (int r = 0; r < RING; ++r) {
                compute(r, kb + r); __builtin_amdgcn_sched_barrier(0); load_w(r, kb + r + RING); __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int r = 0; r < RING - 1; ++r)
            if (kb + r < k1) compute(r, kb + r);
    };
    if (SEG2 && b2 > 0 && OVERLAP2) {
        k_loop(0, b1);
#pragma unroll
        for (int r = 0; r < RING; ++r) load_w(r, b1 + r);          // the ring restarts at the segment boundary (its loads fly
#pragma unroll                                                     //  while segment 2 is being parked)
        for (int j = 0; j < S2P; ++j) seg2_park(j);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        k_loop(b1, blocks);
    } else {
        k_loop(0, blocks);
    }

    // ---- epilogue (bias, activation, residual; 16-byte stores of the transposed accumulators)
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        if (!nvalid[n]) continue;
        const int col = (nt0 + n) * 16 + 4 * g;
        if (col >= p.n_store) continue;
        const f32x4 ebias = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int orow = row0 + 16 * m + c;
            if (orow >= p.M) continue;
            f32x4 v = acc[m][n] + ebias;
            if (p.act == MCG_ACT_SILU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = mcg_silu(v[r]);
            } else if (p.act == MCG_ACT_RELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            if constexpr (RESID) v += eres[m][n];
            float* dst = mcg_gemm_c_ptr(p, orow, nt0 + n, g);
            if (col + 3 < p.n_store) {
                *reinterpret_cast<f32x4*>(dst) = v;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col + r < p.n_store) dst[r] = v[r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// "f32x6" variant: fp32-accurate GEMM on the bf16 matrix pipe (see k_edge_bf16_w64 in mcg_edge_bf16.hip).  Every fp32
// operand is the exact sum of three bf16 parts; the six partial products of weight >= 2^-16 are accumulated in fp32.
// The weights come pre-split ("B-pack16x3": [k-block][part][n-tile][lane][8], host side below).  The activation
// rows are split ONCE per workgroup: the four waves (which share the same 32 rows) each load and split a quarter
// of the 32 x 32 block and publish the parts as MFMA fragments through LDS - one barrier per 32-k block.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

template <int RN>
__global__ __launch_bounds__(256) void mcg_gemm_x6_kernel(McgGemmArgs p) {
    __shared__ __attribute__((aligned(16))) uint16_t a_lds[2 * 2 * 3 * 64 * 8];      // [2][row tile][part][lane][8] = 12 KiB
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c = lane & 15;
    // a workgroup = 32 rows x (4 waves x RN column tiles); unlike mcg_gemm_kernel all four waves MUST share the row
    // block (they split it together), so the grid is (row blocks) x (groups of 4 wave columns)
    const int wave_cols = (p.n_tiles + RN - 1) / RN;
    const int col_groups = (wave_cols + 3) / 4;
    const int blk = mcg_xcd_remap(blockIdx.x, gridDim.x);
    const int row0 = (blk / col_groups) * 32;
    const int wcol = (blk % col_groups) * 4 + wid;
    const bool wave_live = wcol < wave_cols;
    const int nt0 = (wave_live ? wcol : wave_cols - 1) * RN;
    bool nvalid[RN];
    int ncl[RN];
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        nvalid[n] = wave_live && nt0 + n < p.n_tiles;
        ncl[n] = nt0 + n < p.n_tiles ? n : 0;
    }
    f32x4 acc[2][RN];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < RN; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 ebias[RN];
    f32x4 eres[2][RN];
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        const int col = (nt0 + ncl[n]) * 16 + 4 * g;
        ebias[n] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int orow = row0 + 16 * m + c;
            eres[m][n] = (p.resid && orow < p.M && col + 3 < p.n_store) ? *reinterpret_cast<const f32x4*>(p.resid + (size_t)orow * p.ldr + col)
                                                                        : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    // my quarter of the 32 x 32 activation block: row 8*wid + lane/8, k = 4*(lane%8) .. +3 of the block
    const int my_row = 8 * wid + (lane >> 3), my_k = 4 * (lane & 7);
    const int src_row = row0 + my_row < p.M ? row0 + my_row : p.M - 1;
    // where those 4 values live in fragment layout: tile my_row/16, fragment lane (k/8)*16 + row%16, element k%8
    const int frag_off = (((my_row >> 4) * 3) * 64 + ((my_k >> 3) * 16 + (my_row & 15))) * 8 + (my_k & 7);

    const uint16_t* bseg = reinterpret_cast<const uint16_t*>(p.Bp);
    int stage = 0;                       // running k-block counter across both K segments (LDS ring phase)
#pragma unroll 1
    for (int seg = 0; seg < 2; ++seg) {
        const float* A = seg == 0 ? p.A1 : p.A2;
        const int K = seg == 0 ? p.K1 : p.K2;
        const int lda = seg == 0 ? p.lda1 : p.lda2;
        if (K == 0) continue;
        const int blocks = mcg_kblocks16(K);
        const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A), 0, 0xffffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(bseg), 0, 0xffffffff, 0x00020000);
        const unsigned oa = (unsigned)(src_row * lda + my_k) * 4u;
        unsigned obn[RN];
#pragma unroll
        for (int n = 0; n < RN; ++n) obn[n] = (unsigned)((nt0 + ncl[n]) * 64 + lane) * 16u;
        const int part_bytes = p.n_tiles * 64 * 16;
        auto ld = [](const __amdgpu_buffer_rsrc_t& r, unsigned v, int so) { return __builtin_amdgcn_raw_buffer_load_b128(r, (int)v, so, 0); };
        auto load_a = [&](int kb) { return __builtin_bit_cast(f32x4, ld(rs_a, oa, 128 * (kb < blocks ? kb : blocks - 1))); };
        bf16x8 Br[2][3][RN];
        auto load_b = [&](int slot, int kb) {
            kb = kb < blocks ? kb : blocks - 1;
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int n = 0; n < RN; ++n) Br[slot][q][n] = __builtin_bit_cast(bf16x8, ld(rs_b, obn[n], (kb * 3 + q) * part_bytes));
        };
        // split 4 fp32 values into three bf16 parts and publish them into ring half `half`
        auto split_store = [&](f32x4 v, int half) {
            uint16_t* dst = a_lds + half * (2 * 3 * 64 * 8) + frag_off;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                bf16x4 part;
#pragma unroll
                for (int j = 0; j < 4; ++j) part[j] = (__bf16)v[j];
                *reinterpret_cast<bf16x4*>(dst + q * 64 * 8) = part;
                if (q < 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] -= (float)part[j];
                }
            }
        };
        // prologue of the segment: block 0's A parts, B of blocks 0 and 1
        __syncthreads();                                   // previous segment's last reads of the ring are done
        split_store(load_a(0), stage & 1);
        f32x4 a_pref = load_a(1);                          // activation quarter-block, fetched TWO blocks ahead of its split
        load_b(0, 0);
        load_b(1, 1);
        auto block = [&](int slot, int kb) {
            const int half = (stage + kb) & 1;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("s_barrier" ::: "memory");               // A parts of block kb visible; other half free
            const f32x4 an = a_pref;
            a_pref = load_a(kb + 2);
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8* la = reinterpret_cast<const bf16x8*>(a_lds) + half * (2 * 3 * 64) + lane;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                bf16x8 af[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) af[q] = la[(m * 3 + q) * 64];
                // weight part q meets activation parts 0 .. 2-q (the six products of weight >= 2^-16);
                // transposed accumulators: weights are the MFMA A operand (see mcg_gemm_kernel)
#pragma unroll
                for (int q = 0; q < 3; ++q)
#pragma unroll
                    for (int r = 0; r < 3 - q; ++r)
#pragma unroll
                        for (int n = 0; n < RN; ++n) acc[m][n] = mcg_mfma_bf16(Br[slot][q][n], af[r], acc[m][n]);
            }
            __builtin_amdgcn_sched_barrier(0);
            load_b(slot, kb + 2);
            __builtin_amdgcn_sched_barrier(0);
            split_store(an, half ^ 1);
            __builtin_amdgcn_sched_barrier(0);
        };
        int kb = 0;
#pragma unroll 1
        for (; kb + 2 <= blocks; kb += 2) { block(0, kb); block(1, kb + 1); }
        if (kb < blocks) block(0, kb);
        stage += blocks;
        bseg += mcg_pack16x3_elems(K, p.n_tiles);
    }
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        if (!nvalid[n]) continue;
        const int col = (nt0 + n) * 16 + 4 * g;
        if (col >= p.n_store) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int orow = row0 + 16 * m + c;
            if (orow >= p.M) continue;
            f32x4 v = acc[m][n] + ebias[n];
            if (p.act == MCG_ACT_SILU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = mcg_silu(v[r]);
            } else if (p.act == MCG_ACT_RELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            v += eres[m][n];
            float* dst = p.C + (size_t)orow * p.ldc + col;
            if (col + 3 < p.n_store) {
                *reinterpret_cast<f32x4*>(dst) = v;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col + r < p.n_store) dst[r] = v[r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// One wave tile of the fp32 node GEMMs: MR row tiles of 16 x RN column tiles, both K segments, epilogue.  Shared by
// mcg_gemm_kernel (MR = 2, no gather, C through mcg_gemm_c_ptr) and mcg_gemm16_kernel.
//
// ONE operand pipeline per launch.  There is at most one wave per SIMD on the small node GEMMs, so nothing but the wave's own
// MFMAs covers a load: every operand that is first asked for at a K seam (the K % 16 tail steps, the first groups of
// segment 2, the gather table) costs a whole round trip to a cold L2 with the matrix pipe idle.  So
//   * a2_rows is read next to the row clamp, the tail steps' operands (MR x NS A scalars and RN B scalars per step, at most
//     three steps per segment) are requested at the head of the kernel and wait in registers for their seam;
//   * the ring is RING 16-k groups deep (slot = a compile-time constant: a runtime slot turns the ring into a scratch
//     array).  Segment 1 is FRONT-padded to a whole number of ring trips: group j sits in slot (j + s0) % RING with
//     s0 = (RING - G1 % RING) % RING, so only the first trip has empty slots (their MFMAs are skipped, their loads are not:
//     a branch around MFMAs costs nothing, a branch around loads makes the wait-count pass assume the shorter queue and wait
//     for younger loads) and segment 1 always ends on slot RING - 1.  Its LAST trip therefore refills slot i with group i of
//     segment 2 right behind compute(i): segment 2 starts on a full ring, RING - 1 compute blocks ahead as in the steady
//     state.  The trips are peeled explicitly (first | steady loop | last, with and without a segment 2);
//   * bias and residual are requested BEHIND the initial ring fill: the vector-memory counter retires in order, so in front
//     of it they sat between the first MFMA and its operands.
// The k order of every output element is unchanged: segment 1 groups ascending, its tail steps, segment 2 groups, its tail
// steps; the gather sum is ((a + b) + c) + d; bias after the accumulation, SiLU / ReLU, then the residual.
template <int RN, int GATHER, int MR, int RING, bool C_PTR>
__device__ __forceinline__ void mcg_gemm_f32_tile(const McgGemmArgs& p, int row0, int nt0) {
    constexpr int NS = GATHER >= 2 ? GATHER : 1;          // rows of A2 summed per row of segment 2
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, c = lane & 15;
    int orow[MR], rA[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        orow[m] = row0 + 16 * m + c;
        rA[m] = orow[m] < p.M ? orow[m] : p.M - 1;        // clamp: results of padded rows are dropped
    }
    int4 sl[MR];                                          // the gather table, a whole segment 1 ahead of its use
    if constexpr (GATHER >= 2) {
#pragma unroll
        for (int m = 0; m < MR; ++m) sl[m] = p.a2_rows[rA[m]];
    }
    bool nvalid[RN];
    int ncl[RN];            // column-tile offset clamped into range (results of invalid tiles are dropped)
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        nvalid[n] = nt0 + n < p.n_tiles;
        ncl[n] = nvalid[n] ? n : 0;
    }
    // Accumulators are kept TRANSPOSED (weights as the MFMA A operand, activations as B: the two operands have
    // the same lane layout, so this is just the argument order): lane (c, g) of tile (m, n) then holds output
    // row row0 + 16m + c, columns 16(nt0+n) + 4g .. +3 - four consecutive floats, so bias, residual and the
    // result move as 16-byte vectors (6 stores per wave tile instead of 24 dword stores).
    f32x4 acc[MR][RN];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < RN; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int G1 = p.K1 / 16, T1 = (p.K1 - 16 * G1) / 4;  // full 16-k groups and 4-k tail steps of each segment
    const int G2 = p.K2 / 16, T2 = (p.K2 - 16 * G2) / 4;
    const int gbytes = p.n_tiles * 1024;                  // one group of the pack; a tail step is a quarter of it
    const int b2off = (p.K1 / 4) * p.n_tiles * 256;       // segment 2's pack behind segment 1's (mcg_pack4_floats, in bytes)
    // operand addresses = buffer descriptor (SGPRs) + one 32-bit lane offset + a scalar group offset: with
    // 64-bit per-lane pointers every load of the loop costs a 64-bit VALU add, and on gfx950 VALU issue time
    // adds to fp32-MFMA time
    const __amdgpu_buffer_rsrc_t rs_a1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A1), 0, 0xffffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_a2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A2), 0, 0xffffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.Bp), 0, 0xffffffff, 0x00020000);
    // the RING's descriptors: zero records for a segment without a full group - its (still unconditional) loads then fetch
    // nothing and return 0.  A branch around ring loads instead would leave the ring with one definition per path: the
    // copies that join them wait for every load in flight, i.e. drain the ring at the seam.
    // (all ones or zero, by one scalar shift of -G written as asm: however it is spelled in C++, hipcc makes it a select and builds the
    //  word in a VGPR, and a descriptor that is not in SGPRs turns every load into a waterfall loop)
    int n1, n2;
    asm("s_ashr_i32 %0, %1, 31" : "=s"(n1) : "s"(-G1) : "scc");
    asm("s_ashr_i32 %0, %1, 31" : "=s"(n2) : "s"(-G2) : "scc");
    const __amdgpu_buffer_rsrc_t rg_a1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A1), 0, n1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rg_b1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.Bp), 0, n1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rg_a2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A2), 0, n2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rg_b2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.Bp), 0, n2, 0x00020000);
    auto ld4 = [](const __amdgpu_buffer_rsrc_t& r, unsigned v, int so) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)v, so, 0)); };
    auto ld1 = [](const __amdgpu_buffer_rsrc_t& r, unsigned v, int so) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)v, so, 0)); };
    unsigned oa1[MR], ob[RN];
#pragma unroll
    for (int m = 0; m < MR; ++m) oa1[m] = (unsigned)(rA[m] * p.lda1 + 4 * g) * 4u;
#pragma unroll
    for (int n = 0; n < RN; ++n) ob[n] = (unsigned)((nt0 + ncl[n]) * 256 + lane * 4) * 4u;

    // ---- tail steps: lane group g holds k = 16 G + 4 st + g (scalar operands; the B line of step st is a quarter group)
    float ta1[3][MR], tb1[3][RN], ta2[3][MR][NS], tb2[3][RN];
#pragma unroll
    for (int st = 0; st < 3; ++st) {
#pragma unroll
        for (int n = 0; n < RN; ++n) tb1[st][n] = tb2[st][n] = 0.f;
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            ta1[st][m] = 0.f;
#pragma unroll
            for (int q = 0; q < NS; ++q) ta2[st][m][q] = 0.f;
        }
    }
#pragma unroll
    for (int st = 0; st < 3; ++st)
        if (st < T1) {
#pragma unroll
            for (int m = 0; m < MR; ++m) ta1[st][m] = ld1(rs_a1, oa1[m] - 12u * g, (16 * G1 + 4 * st) * 4);
#pragma unroll
            for (int n = 0; n < RN; ++n) tb1[st][n] = ld1(rs_b, ob[n] >> 2, G1 * gbytes + st * (gbytes >> 2));
        }

    // ---- the ring.  Loads are UNCONDITIONAL (group index and column tile clamped): a runtime "load or zero" select makes
    //      hipcc branch around every load and drain vmcnt(0) behind it.
    f32x4 Ar[RING][MR][NS], Br[RING][RN];
    unsigned oa2[MR][NS];
    auto load1 = [&](int slot, int q) {
#pragma unroll
        for (int m = 0; m < MR; ++m) Ar[slot][m][0] = ld4(rg_a1, oa1[m], 64 * q);
#pragma unroll
        for (int n = 0; n < RN; ++n) Br[slot][n] = ld4(rg_b1, ob[n], q * gbytes);
    };
    auto load2 = [&](int slot, int q) {
        q = q < G2 ? q : G2 - 1;
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int s = 0; s < NS; ++s) Ar[slot][m][s] = ld4(rg_a2, oa2[m][s], 64 * q);
#pragma unroll
        for (int n = 0; n < RN; ++n) Br[slot][n] = ld4(rg_b2, ob[n], b2off + q * gbytes);
    };
    auto mfmas = [&](int slot, const f32x4 (&a)[MR]) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int n = 0; n < RN; ++n) acc[m][n] = mcg_mfma(Br[slot][n][s], a[m][s], acc[m][n]);
    };
    auto compute1 = [&](int slot) {
        f32x4 a[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) a[m] = Ar[slot][m][0];
        mfmas(slot, a);
    };
    auto compute2 = [&](int slot) {
        f32x4 a[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            a[m] = Ar[slot][m][0];
#pragma unroll
            for (int s = 1; s < NS; ++s) a[m] = a[m] + Ar[slot][m][s];        // ((a + b) + c) + d: slot order, fixed
        }
        mfmas(slot, a);
    };
    const int s0 = G1 > 0 ? (RING - G1 % RING) % RING : RING;         // empty slots in front of segment 1's first trip
    // (readfirstlane: hipcc takes this clamp through the VALU - a saturating subtract - and would then walk every load of the
    //  fill in a waterfall loop.  Slot by slot: the wait counts in front of the last trip's MFMAs are the worst case over the
    //  paths that reach it, one of them straight from here - the fill keeps the load order of a trip)
#pragma unroll
    for (int i = 0; i < RING; ++i) { load1(i, __builtin_amdgcn_readfirstlane(i > s0 ? i - s0 : 0)); __builtin_amdgcn_sched_barrier(0); }
    __builtin_amdgcn_sched_barrier(0);

    // ---- epilogue operands: behind the ring fill, a whole K loop ahead of their use
    f32x4 ebias[RN], eres[MR][RN];
#pragma unroll
    for (int n = 0; n < RN; ++n) {
        const int col = (nt0 + ncl[n]) * 16 + 4 * g;
        ebias[n] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < MR; ++m)
            eres[m][n] = (p.resid && orow[m] < p.M && col + 3 < p.n_store) ? *reinterpret_cast<const f32x4*>(p.resid + (size_t)orow[m] * p.ldr + col)
                                                                            : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- segment 2's rows (the first use of the gather table: it was the first load of the kernel) and its tail steps
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        if constexpr (GATHER >= 2) {
            const int rows[4] = {sl[m].x, sl[m].y, sl[m].z, sl[m].w};
#pragma unroll
            for (int s = 0; s < NS; ++s) oa2[m][s] = (unsigned)(rows[s] * p.lda2 + 4 * g) * 4u;
        } else {
            oa2[m][0] = (unsigned)(rA[m] * p.lda2 + 4 * g) * 4u;
        }
    }
#pragma unroll
    for (int st = 0; st < 3; ++st)
        if (st < T2) {
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int s = 0; s < NS; ++s) ta2[st][m][s] = ld1(rs_a2, oa2[m][s] - 12u * g, (16 * G2 + 4 * st) * 4);
#pragma unroll
            for (int n = 0; n < RN; ++n) tb2[st][n] = ld1(rs_b, ob[n] >> 2, b2off + G2 * gbytes + st * (gbytes >> 2));
        }
    __builtin_amdgcn_sched_barrier(0);

    // ---- segment 1
    {
        int b = -s0;                                      // group in slot 0 of the current trip
        // sched_barrier pins "MFMAs of slot i | loads into slot i": left alone, hipcc clusters all the loads at the
        // loop bottom and the first MFMA block then waits for every one of them.
        if (G1 > RING) {
#pragma unroll
            for (int i = 0; i < RING; ++i) {              // first trip: slots below s0 are empty
                if (b + i >= 0) compute1(i);
                __builtin_amdgcn_sched_barrier(0); load1(i, b + RING + i); __builtin_amdgcn_sched_barrier(0);
            }
            b += RING;
            // branch-free body (control flow inside the loop makes hipcc's wait-count pass fall back to
            // vmcnt(0) at the loop head, draining the ring); every group it asks for exists
#pragma unroll 1
            for (; b + RING < G1; b += RING) {
#pragma unroll
                for (int i = 0; i < RING; ++i) {
                    compute1(i); __builtin_amdgcn_sched_barrier(0); load1(i, b + RING + i); __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // last trip (b = G1 - RING; the first one too when G1 <= RING, every slot empty when G1 = 0): the ring moves on to
        // segment 2, slot i to its group i
#pragma unroll
        for (int i = 0; i < RING; ++i) {
            if (b + i >= 0) compute1(i);
            __builtin_amdgcn_sched_barrier(0); load2(i, i); __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int st = 0; st < 3; ++st)
        if (st < T1) {
#pragma unroll
            for (int n = 0; n < RN; ++n)
#pragma unroll
                for (int m = 0; m < MR; ++m) acc[m][n] = mcg_mfma(tb1[st][n], ta1[st][m], acc[m][n]);
        }

    // ---- segment 2: the ring holds its groups 0 .. RING - 1
    if (G2 > 0) {
        int q = 0;
#pragma unroll 1
        for (; q + RING <= G2; q += RING) {
#pragma unroll
            for (int i = 0; i < RING; ++i) {
                compute2(i); __builtin_amdgcn_sched_barrier(0); load2(i, q + RING + i); __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int i = 0; i < RING - 1; ++i)
            if (q + i < G2) compute2(i);
    }
#pragma unroll
    for (int st = 0; st < 3; ++st)
        if (st < T2) {
            float av[MR];
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                av[m] = ta2[st][m][0];
#pragma unroll
                for (int s = 1; s < NS; ++s) av[m] += ta2[st][m][s];
            }
#pragma unroll
            for (int n = 0; n < RN; ++n)
#pragma unroll
                for (int m = 0; m < MR; ++m) acc[m][n] = mcg_mfma(tb2[st][n], av[m], acc[m][n]);
        }

#pragma unroll
    for (int n = 0; n < RN; ++n) {
        if (!nvalid[n]) continue;
        const int col = (nt0 + n) * 16 + 4 * g;
        if (col >= p.n_store) continue;
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            if (orow[m] >= p.M) continue;
            f32x4 v = acc[m][n] + ebias[n];
            if (p.act == MCG_ACT_SILU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = mcg_silu(v[r]);
            } else if (p.act == MCG_ACT_RELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            v += eres[m][n];
            float* dst = C_PTR ? mcg_gemm_c_ptr(p, orow[m], nt0 + n, g) : p.C + (size_t)orow[m] * p.ldc + col;
            if (col + 3 < p.n_store) {
                *reinterpret_cast<f32x4*>(dst) = v;       // (4-byte aligned is enough for a global dwordx4 store)
            } else {                                       // ragged right edge (GCN: 210 columns)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col + r < p.n_store) dst[r] = v[r];
            }
        }
    }
}

// 32-row wave tiles: a 256-thread workgroup owns 32 rows x (4 waves x RN column tiles); C row-major or blocked (mcg_gemm_c_ptr).
template <int RN, int RING = 3>
__global__ __launch_bounds__(256) void mcg_gemm_kernel(McgGemmArgs p) {
    const int wid = threadIdx.x >> 6;
    // waves are numbered linearly over (row block, wave column) so that the grid is exactly
    // ceil(waves / 4) workgroups - a 2-D grid rounds each row block up to whole workgroups and
    // can push a 243-workgroup problem over the 256-CU edge into a second round.
    const int wave_cols = (p.n_tiles + RN - 1) / RN;
    const int nblk = p.gemm_blocks > 0 ? p.gemm_blocks : (int)gridDim.x;        // (+ side-job workgroups behind them)
    if ((int)blockIdx.x >= nblk) { mcg_gemm_side_job(p, (int)blockIdx.x - nblk); return; }
    const int wlin = mcg_xcd_remap(blockIdx.x, nblk) * 4 + wid;
    if (wlin >= ((p.M + 31) / 32) * wave_cols) return;
    mcg_gemm_f32_tile<RN, 0, 2, RING, true>(p, (wlin / wave_cols) * 32, (wlin % wave_cols) * RN);
}

// ---------------------------------------------------------------------------------------------
// 16-row variant for the node GEMMs (M = 1.7k .. 7k rows): a wave owns MR 16-row tiles x RN column tiles.
// With 32-row wave tiles the three GEMMs of a GCL layer quantise badly on 1024 SIMDs at M = 1728 (K = 840,
// N = 432: 756 waves of 840 MFMAs = 11.2 us of serial chain on 74 % of the SIMDs); 16 x 3 tiles give 972 waves
// of 630 MFMAs (8.4 us), 16 x 6 the same for N = 864.  Same operand packs, ring discipline and transposed
// accumulators as mcg_gemm_kernel.  GATHER: segment-2 rows are read as the sum of 2 / 3 / 4 rows (see a2_rows).
template <int RN, int GATHER, int MR = 1, int RING = 3>       // GATHER 0 / 2 / 3 / 4 rows summed per A2 row; MR row tiles of 16 per wave
__global__ __launch_bounds__(256) void mcg_gemm16_kernel(McgGemmArgs p) {
    if ((int)blockIdx.x >= p.gemm_blocks) { mcg_gemm_side_job(p, (int)blockIdx.x - p.gemm_blocks); return; }
    const int wid = threadIdx.x >> 6;
    const int wave_cols = (p.n_tiles + RN - 1) / RN;
    const int wlin = mcg_xcd_remap(blockIdx.x, p.gemm_blocks) * 4 + wid;
    if (wlin >= ((p.M + 16 * MR - 1) / (16 * MR)) * wave_cols) return;
    mcg_gemm_f32_tile<RN, GATHER, MR, RING, false>(p, (wlin / wave_cols) * 16 * MR, (wlin % wave_cols) * RN);
}
