/* libmlconfgen_hip.so - C ABI of the MI355X (gfx950) denoising hot path of mlconfgen.
 *
 * The reference (Membrizard/ml_conformer_generator @ 2025-07-04) is pure Python/PyTorch and has no
 * FFI; its operator boundary is the pair of module-call seams that its own ONNX export treats as
 * operators.  Each entry point below names the reference interface it
 * replaces.  Plain pointers and sizes only; every float buffer is fp32, row-major, contiguous and
 * lives in DEVICE memory unless the name ends in `_host`.  `stream` is a hipStream_t (0 = default).
 * All functions return 0 on success (MCG_OK) or a non-zero code; mcg_last_error() gives the text.
 * No global mutable state except the opaque handles.  Behaviour is chosen through arguments: `mcg_plan_opts`
 * (per plan), `mcg_egnn_set_precision` / `mcg_egnn_set_option` (per model), `mcg_plan_set_latency_mode`.  Two PROCESS
 * switches remain, read from the environment, neither needed for normal operation:
 *   MCG_GRAPH=0     plain launches instead of the captured HIP graph per denoiser call (read once, on first use)
 *   MCG_VERBOSE=1   graph capture diagnostics on stderr
 * (Python side: MCG_LIB_PATH = alternative library file, MCG_FORCE_COLLECTIVE=1 = run the final gather on a 1-rank
 * group.)  Threading: like the reference (single Python thread, one stream) - a handle carries workspace, so one
 * mcg_plan / mcg_gcn must not run on two host threads or two streams at once; different handles are independent,
 * mcg_egnn weights are read-only after creation (mcg_egnn_set_precision / mcg_egnn_set_option excepted) and may be
 * shared by several plans.  mcg_last_error() is thread-local.
 * Streams: an entry with a `stream` argument puts all of its device work on that stream - or on internal non-blocking streams
 * ordered behind it by events and joined back into it - and returns without waiting for it; none of it goes through, or waits
 * for, the legacy default stream.  A plan's graph is captured on the plan's own stream and replayed on `stream`.  A handle
 * remembers its last call by an event recorded on that call's stream: mcg_plan_destroy, mcg_gcn_check and a regrowth of the
 * GCN workspace wait for that event, not for the device.  mcg_gcn_destroy waits for it before the workspace goes back to the
 * pool, and then - like mcg_egnn_destroy - returns the weights to the driver, which waits for the whole device.  (The entries
 * that block the host: INTEGRATION.md section 4.)
 */
#ifndef MLCONFGEN_HIP_H
#define MLCONFGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcg_egnn mcg_egnn;   /* packed EGNN weights (one per checkpoint)            */
typedef struct mcg_plan mcg_plan;   /* batch geometry + workspace (one per batch of sizes)  */
typedef struct mcg_gcn mcg_gcn;     /* packed AdjMatSeer weights + workspace                */

const char* mcg_last_error(void);
int mcg_abi_version(void);

/* ---- EGNN weights.  Replaces `EquivariantDiffusion.load_state_dict(...)` of the dynamics
 * (conformer_generator.py:90-95).  `tensors_host` are HOST pointers to the reference-layout
 * fp32 tensors ([out,in] row-major, as nn.Linear stores them) in this order:
 *   embedding.weight, embedding.bias, embedding_out.weight, embedding_out.bias, then for each
 *   block k: gcl_0{edge_mlp.0.w, .0.b, edge_mlp.2.w, .2.b, node_mlp.0.w, .0.b, node_mlp.2.w, .2.b,
 *   att_mlp.0.w, att_mlp.0.b}, gcl_1{same 10}, gcl_equiv{coord_mlp.0.w, .0.b, .2.w, .2.b, .4.w}
 * (n_tensors = 4 + 25*n_blocks; hidden must be 420).  The library repacks them into MFMA
 * fragment order and uploads them. */
int mcg_egnn_create(const float* const* tensors_host, int n_tensors, int hidden, int n_blocks, mcg_egnn** out);
void mcg_egnn_destroy(mcg_egnn* m);
/* mode 0 (default): exact fp32 MFMA everywhere.
 * mode 1 "bf16":  the MFMA operands of the EGNN contractions are rounded to bf16 (fp32 accumulate, fp32
 *                 coordinates / aggregates / epilogues) - BASELINE.json configs[4].
 * mode 2 "f32x6": fp32-accurate edge-MLP contraction on the bf16 matrix pipe: each fp32 operand is carried as the
 *                 exact sum of three bf16 parts and the six partial products of weight >= 2^-16 are accumulated
 *                 in fp32 (dropped terms <= 2^-23 relative); everything else as mode 0.  Uses edge_mt = 4 plans
 *                 (other plans run the exact kernels). */
int mcg_egnn_set_precision(mcg_egnn* m, int mode);
/* Model-level measurement options (defaults in brackets; none is needed for normal operation):
 *   MCG_OPT_X6_GEMM     [1]  f32x6 mode: 1 = node-side GEMMs on the split-operand kernel too, 0 = exact fp32 GEMMs
 *   MCG_OPT_GEMM_RN     [0]  wave tile width (column tiles) of the 32-row node GEMM kernel: 0 = cost model, 1..3
 *   MCG_OPT_GEMM_X6_RN  [0]  same for the split-operand GEMM kernel
 *   MCG_OPT_GEMM_BF16_LDS [0] bf16 mode: 0 = the LDS-staged 9-wave node GEMM from 80 row blocks (2 560 atoms) on, 1 = never (32-row kernel),
 *                            2 = whenever its shape limits allow (results are bit-identical either way)
 *   MCG_OPT_NODE_FUSED  [0]  bf16 mode: the node phase of a GCL layer (node MLP + the next edge layer's first-layer projections) as ONE
 *                            launch: 0 = from 32 row blocks (1 024 atoms) on, 1 = never (three launches),
 *                            2 = whenever the fused launch can run (results are bit-identical either way).  It can run only on
 *                            plans of 64-row units (edge_mt = 4) whose atoms span at most 2 units, with MCG_OPT_GEMM_BF16_LDS != 1,
 *                            on the bf16 gather path (the node GEMM sums an atom's per-unit partial rows itself: not in
 *                            mcg_egnn_gcl_debug, which materialises the aggregate) */
enum { MCG_OPT_X6_GEMM = 1, MCG_OPT_GEMM_RN = 2, MCG_OPT_GEMM_X6_RN = 3, MCG_OPT_GEMM_BF16_LDS = 4, MCG_OPT_NODE_FUSED = 5 };
/* Both setters may be called at any time between denoiser calls: a plan that has already captured its launches as a HIP
 * graph re-captures on its next call (the graph is keyed by the model's option epoch). */
int mcg_egnn_set_option(mcg_egnn* m, int option, int value);

/* Measurement / test hook: node and GCN GEMM launches ISSUED (plainly or into a graph capture) by this process since the
 * last reset, counts_host[family * 8 + rn] with family 0 = 32-row fp32 kernel, 1 = 32-row bf16 kernel, 2 = 16-row-tile fp32
 * kernel, 3 = split-operand kernel and rn = column tiles per wave (family 1: slot 7 = the LDS-staged 9-wave bf16 kernel, slot 6 = the
 * fused node launch of MCG_OPT_NODE_FUSED) - how a
 * test sees that an option changed launch shapes. */
int mcg_debug_gemm_launches(int64_t* counts_host, int reset);

/* ---- Kernel-level pin of the node / GCN GEMMs (csrc/mcg_gemm.hip): ONE launch of one launcher on the caller's data.
 *   C[M, n_store] = act(A1[M,K1] W1^T + G(A2)[M,K2] W2^T + bias) + resid,  W = [W1 | W2] = w_host[n_out][K1 + K2] (nn.Linear
 * layout, HOST memory); rows >= M and columns >= n_store of C are not written.  G = identity, or (a2_rows set) the sum of the
 * first a2_nsum (2..4) of rows a2_rows[r][0..3] of A2 in slot order, ((a + b) + c) + d in fp32, followed in the Bf16 family
 * only by an fp32 division by 100.  Side job (side_x set): side_x[v][0..2] += (((u[s0] + u[s1]) + u[s2]) + u[s3]) / 100 with
 * s = side_slots[v][0..3] and u = side_u[.][4], v < side_M; component 3 is not touched.
 * mcg_debug_gemm packs the weight with the library's own packer for the family, pads the bias to 16 * n_tiles
 * (n_tiles = ceil(n_out / 16)), uploads both through the library's device-memory pool, calls the real launcher with
 * (rn, mr, deep, lds) exactly as given, synchronises `stream`, frees, and reports in *ran_host the template instantiation
 * that ran.  Every contract of the kernels is checked on the HOST first (MCG_ERR_ARG and mcg_last_error() text, no device
 * call made), so a caller cannot launch out of contract:
 *   - d, ran_host, w_host, A1, C not NULL; family, act, c_blocked, deep, lds in range; reserved zero;
 *   - M >= 1, n_out >= 1, 1 <= n_store <= 16 * n_tiles; K1 >= 4, K1 % 4 == 0, K2 >= 0, K2 % 4 == 0, A2 set iff K2 > 0;
 *     every buffer below 2^29 floats (32-bit byte offsets inside the kernels);
 *   - leading dimensions are multiples of 4 and cover what the chosen kernel reads, checked against the buffer sizes the
 *     descriptor states (in floats): lda >= K and a_floats >= (rows - 1) * lda + R(K), rows = M (a2_src_rows for a gathered
 *     A2), with R(K) = K for the fp32 families and R(K) = 32 * ceil(K / 32) for MCG_GEMM_BF16 / MCG_GEMM_X6, whose kernels
 *     read every row up to the next multiple of 32: the caller provides up to 28 FINITE floats behind the K real ones of
 *     every row (the next row's data will do; the last row needs them inside the buffer), which zero weights cancel;
 *     resid: n_store % 4 == 0, ldr >= n_store, resid_floats >= (M - 1) * ldr + n_store;  C: ldc >= n_store and
 *     c_floats >= (M - 1) * ldc + n_store, or c_blocked (below) and c_floats >= 896 * M;
 *   - a gather only with K2 > 0, a2_nsum in 2..4 and a2_src_rows >= 1, and only on MCG_GEMM_F32ROWS16 (sums 2, 3 or 4 rows)
 *     and MCG_GEMM_BF16 (sums 2, or 4 for a2_nsum 3 and 4: the unused slots must name a zero row); a2_nsum = 0 without one;
 *   - a side job (side_x, side_u, side_slots all set, side_M >= 1, side_u_rows >= 1) on every family but MCG_GEMM_X6;
 *   - c_blocked (C[part][14 k-blocks][8 pieces][M rows][4], column = 432 part + 32 k-block + 4 piece + (0..3)) only on
 *     MCG_GEMM_F32 / MCG_GEMM_BF16 and only with n_tiles == 54;
 *   - rn: 0 (the launcher's own choice) .. 3 for MCG_GEMM_F32 / MCG_GEMM_BF16 / MCG_GEMM_X6 (mr = deep = 0 there); for
 *     MCG_GEMM_F32ROWS16 a tile the launcher has an instantiation for: mr 1 with rn 1, 2, 3 or 6, mr 2 with rn 2 or 3, deep
 *     only with mr 1 and rn 1 or 2;  lds (MCG_OPT_GEMM_BF16_LDS: 0 automatic, 1 never, 2 = the LDS-staged kernel if the shape
 *     fits it, else the 32-row kernel) only on MCG_GEMM_BF16.
 * Then, still before the launch, the slot tables are read back and every slot a kernel will read (all four of a side-job
 * entry, the summed ones of a gather) must name a row inside its buffer. */
enum { MCG_GEMM_F32 = 0, MCG_GEMM_F32ROWS16 = 1, MCG_GEMM_BF16 = 2, MCG_GEMM_X6 = 3 };                 /* family = launcher */
enum { MCG_GEMM_KERNEL_F32 = 1, MCG_GEMM_KERNEL_F32ROWS16 = 2, MCG_GEMM_KERNEL_BF16 = 3, MCG_GEMM_KERNEL_BF16_LDS = 4,
       MCG_GEMM_KERNEL_X6 = 5 };
enum { MCG_GEMM_PACK4 = 0, MCG_GEMM_PACK16 = 1, MCG_GEMM_PACK16X3 = 2 };
typedef struct mcg_gemm_desc {
    const float* A1;             /* device [M][lda1] */
    const float* A2;             /* device [M or a2_src_rows][lda2], NULL when K2 = 0 */
    const float* bias;           /* device [n_out] or NULL */
    const float* resid;          /* device [M][ldr] or NULL */
    float* C;                    /* device */
    const int32_t* a2_rows;      /* device [M][4] or NULL */
    const float* side_u;         /* device [side_u_rows][4] */
    const int32_t* side_slots;   /* device [side_M][4] */
    float* side_x;               /* device [side_M][4] */
    const float* w_host;         /* HOST [n_out][K1 + K2] */
    int64_t a1_floats, a2_floats, resid_floats, c_floats;      /* sizes of the buffers behind A1, A2, resid, C */
    int32_t lda1, lda2, ldr, ldc;
    int32_t M, K1, K2, n_out, n_store;
    int32_t act;                 /* 0 none, 1 SiLU, 2 ReLU */
    int32_t a2_nsum, a2_src_rows, side_M, side_u_rows, c_blocked;
    int32_t family, rn, mr, deep, lds;
    int32_t reserved[4];         /* must be zero */
} mcg_gemm_desc;
/* kernel = MCG_GEMM_KERNEL_*, then its template arguments (0 where the template has none): mcg_gemm_kernel<RN, RING>,
 * mcg_gemm16_kernel<RN, GATHER, MR, RING>, mcg_gemm_bf16_kernel<RN, GATHER>, mcg_gemm_bf16_lds_kernel<GATHER, RESID, SEG2,
 * RING>, mcg_gemm_x6_kernel<RN> */
typedef struct mcg_gemm_ran {
    int32_t kernel, rn, mr, ring, gather, resid, seg2, reserved;
} mcg_gemm_ran;
int mcg_debug_gemm(const mcg_gemm_desc* d, mcg_gemm_ran* ran_host, void* stream);
/* Host only: the operand pack of W = w_host[n_out][K1 + K2] that family reads - `kind` MCG_GEMM_PACK4 (float elements:
 * mcg_gemm_launch / mcg_gemm16_launch), MCG_GEMM_PACK16 (uint16 bf16 bits: mcg_gemm_bf16_launch) or MCG_GEMM_PACK16X3
 * (uint16: mcg_gemm_x6_launch) - segment 1 (columns 0 .. K1-1) followed by segment 2, rows >= n_out zero.  *n_elems_host
 * receives the element count; dst_host (NULL = count only) must hold dst_capacity >= that many elements. */
int mcg_debug_gemm_pack(const float* w_host, int n_out, int K1, int K2, int kind, void* dst_host, int64_t dst_capacity,
                        int64_t* n_elems_host);

/* ---- Batch plan.  Replaces the per-call `get_adj_matrix` edge-list rebuild (egnn.py:475,515-541)
 * and the node/edge masks (mol_utils.py:226-252): node_mask[b] is the prefix of n_nodes_host[b]
 * ones, edge_mask = outer product minus diagonal.  edge_mt: 0 = auto, 1 = 16-row edge tiles (exact-fp32 kernels,
 * 16-row bf16 kernel), 4 = 64-row units (bf16 / f32x6 kernels; needs <= 16 atoms' rows per unit). */
int mcg_plan_create(int B, int N, const int32_t* n_nodes_host, int edge_mt, mcg_plan** out);
/* The same with every choice the library would make itself open to the caller (a zero-initialised struct = defaults;
 * `opts` may be NULL):
 *   edge_mt          as above
 *   n_ranges         independent molecule ranges, each running the whole denoiser on its own HIP stream inside
 *                    mcg_egnn_dynamics: 0 = the library's choice (16-row-tile plans: 1 / 2 / 3 / 4 ranges below 3 600 /
 *                    5 200 / 14 000 / from 14 000 edge tiles on; 64-row-unit plans: 2 from 8 192 tiles on), 1..4 given
 *   four_tile_units  workgroups of the exact-fp32 throughput edge kernel that take four 16-row tiles each (the rest take
 *                    ONE tile, its columns split over the 4 waves): 0 = every complete round of the chip (default),
 *                    -1 = none, n > 0 = the first n (rounded up to a multiple of 8, capped at all of them;
 *                    MCG_ALL_FOUR_TILE = all) */
typedef struct mcg_plan_opts {
    int32_t edge_mt;
    int32_t n_ranges;
    int32_t four_tile_units;
    int32_t reserved[5];          /* must be zero */
} mcg_plan_opts;
#define MCG_ALL_FOUR_TILE 0x3fffffff
/* Accepted molecule sizes.  An atom's n - 1 edge rows may run through at most 8 units of 16 * edge_mt rows, which every
 * molecule of up to 7 * 16 * edge_mt + 3 atoms satisfies wherever it stands in the batch:
 *   edge_mt 1 (and 0 = auto, which is 1): 0 .. 115 atoms per molecule;
 *   edge_mt 4:                            0 .. 451 atoms, and no 64-row unit may hold rows of more than 16 atoms (batches
 *                                         with molecules below 6 atoms need edge_mt 1).
 * A larger molecule is refused with MCG_ERR_ARG and a message that names it, before any device call, also where its rows
 * would happen to fit behind the molecules in front of it.  (Which kernels serve which sizes: mcg_debug_route.) */
int mcg_plan_create_ex(int B, int N, const int32_t* n_nodes_host, const mcg_plan_opts* opts, mcg_plan** out);
void mcg_plan_destroy(mcg_plan* p);
/* Plans take their device memory (one block of tables, one of workspace) from a per-device pool inside the library: the
 * blocks of a destroyed plan are handed to the next one instead of going back to the driver, so a caller that meets a new
 * size vector on every call (and evicts an old plan on every call) allocates nothing in steady state.
 * stats_host[4] (may be NULL) = {bytes in use by live plans, bytes cached for reuse, driver allocations so far, pool hits so
 * far} of the current device; trim != 0 first returns every cached block to the driver. */
int mcg_pool_stats(int64_t* stats_host, int trim);
/* Edge-kernel choice (exact-fp32 mode, edge_mt 1): -1 auto - the throughput kernel, whose workgroups take four 16-row
 * tiles each for every complete round of the chip and ONE tile each (columns split over the 4 waves) for the rest, i.e.
 * for the whole of a small batch; 0 = four-tile workgroups only; 1 = the stand-alone column-split kernel with per-wave
 * partial sums (the fallback for plans without workgroup-level tables). */
int mcg_plan_set_latency_mode(mcg_plan* p, int mode);
/* Host-only self-check of the tables mcg_plan_create_ex would build for a device with `cus` compute units (no GPU
 * call; same `opts`): every edge row's (unit, tile, segment) must land in a slot its
 * atom lists, no slot may be shared by two atoms, a four-tile unit parks <= 16 rows, the row table names the right
 * (i, j).  info[8] = {table sets, units, four-tile units, slots, most slots per atom of set 0; units, slots, most slots
 * per atom of set 1 (four-tile units only; zeros when there is one set)}.  Returns MCG_OK or an error with text. */
int mcg_plan_check_tables(int B, int N, const int32_t* n_nodes_host, const mcg_plan_opts* opts, int cus, int32_t* info_host);
/* info[8] = {real nodes, real edges, edge_mt, edge waves, partial slots, B, N, 16-row edge tiles} */
int mcg_plan_info(const mcg_plan* p, int32_t* info_host);
/* number of molecule ranges (HIP streams) the plan actually runs: 1 = unsplit (small batches are never split) */
int mcg_plan_ranges(const mcg_plan* p);

/* ---- Op seam 1: out[B,N,11] = EGNNDynamics.forward(t[B,1], xh[B,N,11], node_mask, edge_mask,
 * context[B,N,3])  (egnn.py:472-513; called from equivariant_diffusion.py:187).  Masks are those of
 * the plan.  Inputs are not modified; `out` may not alias `xh`. */
int mcg_egnn_dynamics(const mcg_egnn* m, mcg_plan* p, const float* t, const float* xh, const float* context,
                      float* out, void* stream);

/* Kernel-level pin: ONE EquivariantBlock (egnn.py:188-222) on compact node arrays
 * h_io[M,420], x_io[M,3], x0[M,3] (M = real nodes of the plan, molecule-major). */
int mcg_egnn_block_debug(const mcg_egnn* m, mcg_plan* p, int block, float* h_io, float* x_io, const float* x0,
                         void* stream);

/* Debug hooks: one GCL layer (egnn.py:70-85) on compact arrays (result stays in the plan), and a
 * copy-out of the plan's internal buffers: which = 0 h[M][432], 1 pab[M][864], 2 agg[M][432],
 * 3 node-MLP hidden[M][432], 4 x[M][4], 5 pab as the bf16 mode's edge_mt = 4 plans store it: piece-major
 * [part a | b][k-block 0..13][piece 0..7][M][4], M * 896 floats (which = 1 copies the first M * 864 of the same buffer,
 * which is the whole of it in the row-major layout of every other plan). */
int mcg_egnn_gcl_debug(const mcg_egnn* m, mcg_plan* p, int layer, const float* h_in, const float* x_in,
                       const float* x0, void* stream);
int mcg_plan_peek(const mcg_plan* p, int which, float* dst, void* stream);
/* Test hooks (additions, ABI version unchanged).  mcg_egnn_gcl_debug_ex: keep_agg = 1 is mcg_egnn_gcl_debug; keep_agg = 0
 * runs the layer as a denoiser call does - the aggregate is gathered by the node GEMM (agg is NOT materialised) and, where
 * MCG_OPT_NODE_FUSED and the plan allow it, the node phase is the one fused launch, which writes no hidden buffer and leaves
 * the NEXT layer's first-layer projections in pab.  ran_host[2] (may be null) = {fused launch ran, pab holds the next layer's
 * projections}.  mcg_egnn_equiv_debug: the coordinate layer of `block` (egnn.py:111-149) on the same compact arrays; apply = 0
 * applies a pending update by a launch of its own, apply = 1 (block + 1 < n_blocks) has it consumed as the side job of the next
 * block's first first-layer GEMM, as a denoiser call does - pab then holds that layer's projections; x' is peek 4.
 * Plans cut into molecule ranges are refused; argument errors return MCG_ERR_ARG without a launch. */
int mcg_egnn_gcl_debug_ex(const mcg_egnn* m, mcg_plan* p, int layer, const float* h_in, const float* x_in,
                          const float* x0, int keep_agg, int32_t* ran_host, void* stream);
int mcg_egnn_equiv_debug(const mcg_egnn* m, mcg_plan* p, int block, const float* h_in, const float* x_in,
                         const float* x0, int apply, void* stream);
/* Test hook: the kernels a denoiser call of model `m` on plan `p` would run, read from the same routing function the
 * launchers use (keep_agg != 0: as mcg_egnn_gcl_debug runs a layer).  Host only: nothing is launched, nothing is written
 * on the device.  A plan cut into molecule ranges reports its first range.  info_host[8] =
 *   [0] edge kernel:            MCG_ROUTE_EDGE_*
 *   [1] first-layer GEMM family: MCG_GEMM_F32 (32-row fp32), MCG_GEMM_F32ROWS16, MCG_GEMM_BF16, MCG_GEMM_X6
 *   [2] aggregate source:       MCG_ROUTE_AGG_*
 *   [3] 1 = the node phase of a GCL layer is the one fused launch (MCG_OPT_NODE_FUSED)
 *   [4] node GEMM family (as [1])
 *   [5] coordinate update:      MCG_ROUTE_COORD_*
 *   [6] most per-unit partial-sum slots any atom has (units of 16 * edge_mt rows; the gathers need <= 4)
 *   [7] most rows of the workgroup-level sums any atom has in the unit tables the route uses; 0 = it uses none (the plan
 *       has no unit tables, or the edge kernel is not MCG_ROUTE_EDGE_EXACT - latency mode 1, bf16, f32x6)
 * MCG_ERR_ARG on a null argument. */
enum { MCG_ROUTE_EDGE_EXACT = 0,       /* exact-fp32 throughput kernel on unit tables (four-tile / quarter-tile units) */
       MCG_ROUTE_EDGE_NS = 1,          /* exact-fp32 column-split kernel, per-tile partial sums: any molecule size */
       MCG_ROUTE_EDGE_BF16ROWS16 = 2,  /* bf16 operands, 16-row tiles */
       MCG_ROUTE_EDGE_W64BF16 = 3,     /* bf16 operands, 64-row units */
       MCG_ROUTE_EDGE_W64X6 = 4,       /* f32x6 split operands, 64-row units */
       MCG_ROUTE_EDGE_INVALID = 5 };   /* exact fp32 on a 64-row plan: the call fails with MCG_ERR_STATE */
enum { MCG_ROUTE_AGG_GATHER_U = 0,     /* node GEMM sums an atom's rows of the workgroup-level sums itself */
       MCG_ROUTE_AGG_GATHER_P = 1,     /* node GEMM sums an atom's (<= 4) per-unit partial rows itself (bf16) */
       MCG_ROUTE_AGG_GATHER_AGG2 = 2,  /* workgroup-level sums materialised by a launch of their own (keep_agg) */
       MCG_ROUTE_AGG_COMBINE = 3 };    /* an atom's (<= 8) per-unit partial rows summed by a launch of their own */
enum { MCG_ROUTE_COORD_PENDING_U = 0, MCG_ROUTE_COORD_PENDING_P = 1,   /* side job of the next first-layer GEMM / output head */
       MCG_ROUTE_COORD_KERNEL = 2 };   /* a launch of its own right behind the edge kernel */
int mcg_debug_route(const mcg_egnn* m, const mcg_plan* p, int keep_agg, int32_t info_host[8]);

/* Measurement hook: the edge-MLP kernel of GCL layer `layer` (equiv = 0, 0..2*n_blocks-1) or of the
 * coordinate update of block `layer` (equiv = 1) launched `iters` times on the plan's current state. */
int mcg_bench_edge(const mcg_egnn* m, mcg_plan* p, int layer, int equiv, int iters, void* stream);
/* Measurement hook: `calls` whole denoiser calls (arguments as mcg_egnn_dynamics) issued as plain launches with every
 * edge-MLP launch bracketed by events that receive the kernel's own begin / end timestamps, i.e. the dominant kernel timed
 * in the context it runs in.  us_host[4] = {mean us of the 18 GCL edge launches per call, mean us of the 9 coordinate-layer
 * ones, how many of each were timed}.  Synchronises `stream`. */
int mcg_bench_edge_incall(const mcg_egnn* m, mcg_plan* p, const float* t, const float* xh, const float* context, float* out,
                          int calls, float* us_host, void* stream);

/* ---- Sampler arithmetic (equivariant_diffusion.py).  randn_x[B,N,3] / randn_h[B,N,8] are RAW
 * standard-normal draws (the caller draws them in the reference's order: x first, then h);
 * masking and centre-of-gravity removal (:56-76) happen inside. */
/* eps[B,N,11] = sample_combined_position_feature_noise (:341-363) */
int mcg_sampler_noise(const mcg_plan* p, const float* randn_x, const float* randn_h, float* eps, void* stream);
/* z <- sample_p_zs_given_zt (:295-339): one network call + ancestral update + mean removal.
 * alpha_ts, c_eps = sigma2_ts/alpha_ts/sigma_t, c_noise = sigma_ts*sigma_s/sigma_t are the fp32
 * scalars of :308-326; t_dev[B] holds t. */
int mcg_sampler_step(const mcg_egnn* m, mcg_plan* p, float* z, const float* context, const float* t_dev,
                     const float* randn_x, const float* randn_h, float alpha_ts, float c_eps, float c_noise,
                     float* eps_hat_scratch, void* stream);
/* x[B,N,3], h[B,N,8] (one-hot, float) = sample_p_xh_given_z0 (:261-285) */
int mcg_sampler_decode(const mcg_egnn* m, mcg_plan* p, const float* z0, const float* context, const float* t_zero_dev,
                       const float* randn_x, float inv_alpha0, float sigma0, float sigma_x, float norm_x, float norm_h,
                       float* eps_hat_scratch, float* x_out, float* h_out, void* stream);
/* mode 0: z = alpha_s*z_known + sigma_s*eps            (merge_fragments :548-559)
 * mode 1: re-noise z_known, align the fixed fragment's centre of mass (:79-105), blend (:489-493) */
int mcg_sampler_blend(const mcg_plan* p, float* z, const float* z_known, const float* fixed_mask, const float* randn_x,
                      const float* randn_h, float alpha_s, float sigma_s, float blend, int mode, void* stream);
/* Keyed raw draws (opt-in `sample_seed`): randn_x[B,N,3], randn_h[B,N,8] of one draw, for the four consumers above, as a
 * function of (seed, sample id, run, draw, atom) only - independent of the molecule's row, B, N or rank.
 * Philox4x32-10 (Salmon et al., SC'11), key (seed & 0xffffffff, seed >> 32), counter
 * (sample_ids_dev[b], draw, atom i within molecule b, (run << 8) | block), block 0..2.  Each block's words (w0,w1,w2,w3)
 * give 4 normals by Box-Muller on (w0,w1) and (w2,w3):
 *   u1 = ((w_even >> 8) + 1) * 2^-24,  u2 = (w_odd >> 8) * 2^-24,  r = sqrt(-2 ln u1),
 *   z_even = r cos(2 pi u2),  z_odd = r sin(2 pi u2);
 * normal q = 4*block + j is channel q (0..2 = x, 3..10 = h; the 12th is discarded).  Padded slots (i >= n_b) are 0.
 * sample_ids_dev: B int64 ids in [0, 2^32), device memory.  `draw` counts the draws of one sampler run from 0 (initial
 * latent), `run` the sampler runs of one generation call (< 2^24).  Null plan / ids / outputs or run >= 2^24:
 * MCG_ERR_ARG, nothing launched.  (Molecule sizes use counter (sample_id, 0, 0, 0xffffffff) on the host.) */
int mcg_sampler_noise_keyed(const mcg_plan* p, uint64_t seed, const int64_t* sample_ids_dev, uint32_t run, uint32_t draw,
                            float* randn_x, float* randn_h, void* stream);

/* ---- Stand-alone aggregate (unsorted_segment_sum of gate*m, egnn.py:49-64,418-437) over the compact
 * real-edge list: node v owns n_rows[v] consecutive rows of m[E_r, D] starting at first_row[v];
 * out[v,:] = sum_j gate[row]*m[row,:] / 100.  HBM-roofline probe; production fuses this. */
int mcg_egnn_aggregate(const float* m, const float* gate, const int32_t* first_row, const int32_t* n_rows, float* out,
                       int n_nodes, int D, void* stream);

/* ---- Op seam 2: AdjMatSeer (adj_mat_seer.py:104-165).  tensors_host order (22):
 *   gcn1..4.linear.{weight,bias}, resize.{weight,bias}, nodes_embedding.weight,
 *   nodes_coord_fc.{weight,bias}, gcn1_dm..gcn3_dm.linear.{weight,bias}, dm_resize.{weight,bias},
 *   dm_nodes_embedding.weight */
int mcg_gcn_create(const float* const* tensors_host, int n_tensors, mcg_gcn** out);
void mcg_gcn_destroy(mcg_gcn* g);
/* logits[B,42,42,5] = adj_mat_seer(elements[B,42] int64, dist_mat[B,42,42], adj_mat[B,42,42]);
 * bond[B,42,42] int8 = argmax over the 5 bond classes (the consumer's reduction, mol_utils.py:210).
 * Either output may be NULL.  The workspace is sized for the largest B seen, zero-filled on `stream`; a larger B first waits
 * (on the host) for the handle's previous call, then takes new blocks from the library's device-memory pool. */
int mcg_gcn_forward(mcg_gcn* g, const int64_t* elements, const float* dist_mat, const float* adj_mat, float* logits,
                    int8_t* bond, int B, void* stream);
/* MCG_ERR_STATE if an element id outside [0, 36) was fed since creation (nn.Embedding would have raised), else MCG_OK.  Blocks
 * the host until the handle's last mcg_gcn_forward has run, on whichever stream that was given, and reads the flag behind it. */
int mcg_gcn_check(mcg_gcn* g);
/* Debug hook: a copy-out of the GCN's workspace as the last mcg_gcn_forward left it, for the first B molecules of that
 * call: which = 0 L_dm[B,42,42] (normalised distance graph), 1 L_adj[B,42,42] (normalised bond graph), 2 the per-atom
 * bottleneck[B,42] (dm_resize), 3 scale[B,42*64] (nodes_coord_fc), 4 the main branch's input e0[B,42,64] (embedding +
 * scale), 5 the last GraphConv's output xb[B*42,2048], 6 res[B,42,42,5] (resize, before symmetrisation).  One
 * device-to-device copy on `stream`; the forward pass is not touched.  MCG_ERR_ARG, nothing copied: a null argument, an
 * unknown `which`, B < 1 or B above what the workspace was last sized for. */
int mcg_gcn_peek(const mcg_gcn* g, int which, int B, float* dst, void* stream);
/* EDM -> GCN hand-off (replaces samples_to_rdkit_mol + prepare_adj_mat_seer_input, utils/mol_utils.py:18-57,146-194,
 * for the tensor part): elements[B,42] int64 (atomic numbers, 0 padded), dist_mat[B,42,42] (distances + I),
 * adj_mat[B,42,42] ({0,1} covalent-radius connectivity + I) from x[B,N,3], h[B,N,8] one-hot and n_nodes[B] (device
 * int32).  Atoms keep their generation order.  dist_mat is the reference's BIT FOR BIT: coordinates through the "%.9f" text
 * round trip (rint(x * 1e9) / 1e9, exact in fp64), fp64 differences / sum / sqrt in `distance_matrix`'s order, ONE rounding
 * to fp32 at the store (utils/mol_utils.py:46-51,129-143,168,176-187); the covalent rule compares in fp64 as well
 * (ABI 4: cov_factor is a double). */
int mcg_handoff(const float* x, const float* h, const int32_t* n_nodes_dev, int B, int N, double cov_factor,
                int64_t* elements, float* dist_mat, float* adj_mat, void* stream);
/* The same with the two RDKit-owned decisions of the reference open to the caller (`canonicalise`,
 * utils/mol_utils.py:110-126: DetermineConnectivity + `_smilesAtomOutputOrder` + RenumberAtoms; the MolGraph adjacency
 * of `prepare_adj_mat_seer_input`, :146-194).  AdjMatSeer is NOT permutation-equivariant (nodes_coord_fc is a dense layer
 * over the position index, adj_mat_seer.py:135-138), so a checkpoint trained on canonical-SMILES order needs that order:
 *   order[B,42] int32 (device; NULL = generation order): order[b][p] = generation index of the atom placed at
 *                position p - the argument of `Chem.RenumberAtoms(mol, order)`; the first n_nodes[b] entries of row b must
 *                be a permutation of 0..n_nodes[b]-1 (out-of-range entries are clamped and reported through
 *                bad_order_flag), the rest is ignored;
 *   conn_in[B,42,42] uint8 (device; NULL = covalent-radius rule d < cov_factor*(r_i + r_j)): symmetric {0,1}
 *                1-order connectivity in GENERATION order (what DetermineConnectivity perceives before renumbering);
 *                the diagonal is ignored, +I is added here; it is permuted with the atoms;
 *   x_out[B,N,3] (NULL = not wanted; may not alias x): the coordinates in the order of the GCN input, zero padded -
 *                the reference's `canonicalised_samples`, whose order the bond write-back and the returned
 *                molecules follow (conformer_generator.py:357-366);
 *   bad_order_flag (device int32, NULL = not wanted): set to 1 if an order entry was out of range; never cleared here.
 * elements / dist_mat / adj_mat come out in the permuted order. */
int mcg_handoff_ex(const float* x, const float* h, const int32_t* n_nodes_dev, int B, int N, double cov_factor,
                   const int32_t* order, const uint8_t* conn_in, int64_t* elements, float* dist_mat, float* adj_mat,
                   float* x_out, int32_t* bad_order_flag, void* stream);
/* The same with the caller's atom decoder (`MLConformerGenerator(atom_decoder=)`): the reference writes
 * atom_decoder[argmax(h)] into the XYZ block of `samples_to_rdkit_mol` (utils/mol_utils.py:41-45), and the atomic number
 * RDKit reads from it is what `MolGraph.elements_vector` embeds and what DetermineConnectivity works from.
 *   class_z[8] int32 (HOST; NULL = the default decoder C N O F P S Cl Br, i.e. mcg_handoff_ex): atomic number of each atom
 *                class.  Every entry must be an element the library knows - B C N O F Si P S Cl As Se Br, each Z < 36 (the
 *                GCN's element embedding) - else MCG_ERR_ARG before any device work.  Two classes may share an element.
 * elements carries these atomic numbers; the covalent-radius rule (conn_in NULL) uses each element's single-bond radius
 * (Cordero 2008). */
int mcg_handoff_elements(const float* x, const float* h, const int32_t* n_nodes_dev, int B, int N, double cov_factor,
                         const int32_t* order, const uint8_t* conn_in, int64_t* elements, float* dist_mat, float* adj_mat,
                         float* x_out, int32_t* bad_order_flag, const int32_t* class_z, void* stream);

/* Bond write-back + validity pre-filter behind the GCN (replaces the tensor half of `redefine_bonds`,
 * utils/mol_utils.py:197-223, and stands in for `standardize_mol(...) is not None`, conformer_generator.py:362-366 /
 * utils/standardizer.py:83-111, which is RDKit sanitisation + MMFF and cannot run without RDKit):
 * bond[B,42,42] int8 = argmax bond classes from mcg_gcn_forward; bond_sym[B,42,42] int8 = its strict lower triangle
 * mirrored, zero outside the molecule's n x n block; valid[B] uint8 = 1 when no atom exceeds its maximum valence and
 * the bond graph is one connected fragment (a labelled PROXY, not RDKit's gate).  Maximum valences by atomic number:
 * B 3, C 4, N 4, O 2, F 1, Si 4, P 5, S 6, Cl 1, As 5, Se 6, Br 1; any other element 0. */
int mcg_bond_writeback(const int8_t* bond, const int64_t* elements, const int32_t* n_nodes_dev, int B, int8_t* bond_sym,
                       uint8_t* valid, void* stream);
/* Inertial fragment matching, the tensor work between its two sampler runs (`inverse_coord_transform`,
 * utils/mol_utils.py:508-524, then `ifm_prepare_fragments_for_merge`, :460-505) in one launch:
 * z_known[B,N,11] = [fixed fragment (ff_x[n_ff,3] | ff_h[n_ff,8]) ; gen_x[B,n_gen,3] @ rotation[B,3,3]^T - shift[B,3] |
 * gen_h[B,n_gen,8]], zero rows up to N; fixed_mask[B,N,1] = 1 on the first n_ff rows.  n_ff + n_gen <= N. */
int mcg_ifm_merge(const float* ff_x, const float* ff_h, int n_ff, const float* gen_x, const float* gen_h, int n_gen,
                  const float* shift, const float* rotation, int B, int N, float* z_known, float* fixed_mask, void* stream);

/* ---- Evaluation (grid half): Gaussian-volume shape Tanimoto of one reference against B
 * candidates in R orientations - `tanimoto_score` (cheminformatics/shape_similarity.py:468-492) for every
 * (candidate, rotation) pair of `evaluate_samples` (cheminformatics/pipeline.py:64-85).
 * ref[n_ref,3]; cand[B,N,3] with n_nodes[B] real atoms; rot[R,9] row-major matrices applied as coord @ M;
 * axes[3,n] = the three linspace axes of the n^3 grid (built by the caller exactly as the reference's
 * `Grid`); f_scratch[n^3]; score[B*R].  A row is scored on its first n_nodes[b] atoms, clamped to [0, N].
 * MCG_ERR_ARG, nothing launched: a null buffer, n_ref outside 1..64, B < 1, N outside 1..64 (a wider row would be scored on
 * its first 64 atoms only), R < 1, n < 2. */
int mcg_shape_tanimoto(const float* ref, int n_ref, const float* cand, const int32_t* n_nodes_dev, int B, int N,
                       const float* rot, int R, const float* axes, int n, float alpha, float amplitude,
                       float* f_scratch, float* score, void* stream);

/* ---- Evaluation (frame half): principal shape frames of B padded molecules of N <= 64 atoms -
 * `get_shape_quadrupole_for_molecule` (cheminformatics/shape_similarity.py:18-202), two launches around the host's 3x3
 * eigen-decomposition (its LAPACK eigenvector signs choose between a frame and its mirror image):
 *   mcg_shape_moments: pass 1 on the input points -> shape centre[B,3] (fp32) and volume[B] (fp64 sum); pass 2 on the
 *                      centred points -> second-moment tensor[B,9] (row-major, fp32, divided by the volume);
 *                      clique_counts[B, n_terms-1] (optional, NULL = not wanted): cliques of order 2..n_terms per molecule.
 *   mcg_shape_frames:  eigvecs[B,9] = V row-major (column j = eigenvector j, as torch.linalg.eigh returns it) of that
 *                      tensor; pass 3 on the rotated points -> main moments[B,3] (descending) and frames[B,N,3] (the
 *                      rotated points, axes permuted to match; zero on padded rows).
 * coords[B,N,3] with n_nodes_dev[b] real atoms (device memory, clamped to [0, N] on the device); both launches build the
 * same neighbour graph (0 < d < neighbour_threshold) from coords.  centre_atoms != 0: the real atoms' mean is subtracted
 * from coords first (evaluate_shape's centring).  Terms in fp32, sums in fp64 per molecule, fixed lane assignment and
 * reduction order: every output is bit-identical run to run and whatever the batch, row or padded width.
 * MCG_ERR_ARG, nothing launched: a null buffer, B < 1, N outside 1..64, n_terms outside 2..8, alpha, amplitude or
 * neighbour_threshold not > 0. */
int mcg_shape_moments(const float* coords, const int32_t* n_nodes_dev, int B, int N, double alpha, double amplitude,
                      float neighbour_threshold, int n_terms, int centre_atoms, float* centre, float* tensor,
                      double* volume, int64_t* clique_counts, void* stream);
int mcg_shape_frames(const float* coords, const int32_t* n_nodes_dev, int B, int N, const float* centre,
                     const float* eigvecs, const double* volume, double alpha, double amplitude, float neighbour_threshold,
                     int n_terms, int centre_atoms, float* moments, float* frames, void* stream);

/* ---- Pose on the reference: the rigid, proper transform that puts each candidate onto the
 * reference conformer's own coordinates, from the frames above and the four-orientation search.
 *   mcg_shape_frames_tf: mcg_shape_frames (same outputs, bit for bit) plus xform[B,12] = M row-major (M = V P: the
 *                        eigenvectors, then the descending-moment axis permutation), then t (atom mean + shape centre):
 *                        frames = (coords - t) @ M on the real rows.  det(M) = +-1.
 *   mcg_shape_overlay:   ref_frame[n_ref,3] / ref_xform[12] (M_r, t_r) and frames[B,N,3] / xform[B,12] (M_s, t_s) from
 *                        mcg_shape_frames_tf.  Handedness: M_s' = M_s diag(1,1,-1) where det(M_s) det(M_r) < 0
 *                        (flipped[b] = 1), else M_s' = M_s.  The frame (coords - t_s) @ M_s' is scored in the four
 *                        orientations rot[4,9] (identity, pi about x, y, z: proper) on the grid axes[3,n] of ref_frame,
 *                        as mcg_shape_tanimoto does (score[B*4], optional: NULL = not wanted; bit-identical to
 *                        mcg_shape_tanimoto on the handedness-fixed frames); best[b] / which[b] = the first maximum.
 *                        pose[B,12] = Q row-major, then d, with Q = M_s' R_which M_r^T (det +1) and d = t_r - t_s @ Q;
 *                        posed[B,N,3] = z_best @ M_r^T + t_r (= coords @ Q + d) on the real rows, zero on padded rows.
 *                        A row whose frame or xform is not finite: NaN best, which = -1, NaN pose and posed rows; the
 *                        other rows are unaffected.  f_scratch[n^3]; one 256-lane workgroup per candidate.
 * MCG_ERR_ARG, nothing launched: a null required buffer, B < 1, N outside 1..64, n_ref outside 3..64 (overlay), n < 2,
 * and the argument errors of mcg_shape_frames. */
int mcg_shape_frames_tf(const float* coords, const int32_t* n_nodes_dev, int B, int N, const float* centre,
                        const float* eigvecs, const double* volume, double alpha, double amplitude,
                        float neighbour_threshold, int n_terms, int centre_atoms, float* moments, float* frames,
                        float* xform, void* stream);
int mcg_shape_overlay(const float* ref_frame, int n_ref, const float* ref_xform, const float* frames, const float* xform,
                      const int32_t* n_nodes_dev, int B, int N, const float* rot, const float* axes, int n, float alpha,
                      float amplitude, float* f_scratch, float* score, float* best, int32_t* which, int32_t* flipped,
                      float* pose, float* posed, void* stream);

/* ---- Refined pose on the reference ("Refined pose"): mcg_shape_overlay, then each of its four
 * starts moved as a rigid body to maximise the first-order Gaussian overlap with the reference,
 * O(y, z) = sum_ij A^2 (pi / (2 alpha))^1.5 exp(-(alpha / 2) |y_i - z_j|^2), by `steps` (0..1024) steps of a
 * normalised-gradient ascent (rotation about the atom centroid along the torque, translation along the force; a step is
 * kept only if O strictly increases).  Takes mcg_shape_overlay's arguments (same meaning) and writes its outputs; then
 *   refine_ws[B*4*12]   work space: per (candidate, start) G row-major, then t, with z' = z @ G + t;
 *   objective[B*4*2]    optional (NULL = not wanted): O before and after the ascent, per start;
 *   start_best[B]       the unrefined best score (mcg_shape_overlay's best, bit for bit);
 *   refined[B]          1 where a refined candidate replaced the start pose: the four refined candidates are scored on
 *                       the reference's grid exactly as mcg_shape_overlay scores the starts (refined_score[B*4],
 *                       optional), and the first maximum replaces the start only if strictly better.  Then best / which /
 *                       pose / posed describe the refined pose: Q = M_s' R_which G M_r^T, d = t_r + t @ M_r^T - t_s @ Q.
 *                       A row that failed in mcg_shape_overlay keeps that entry's outputs (refined 0, NaN objective).
 * Four launches on `stream` (density, overlay, one 256-lane workgroup per (candidate, start), one per candidate); every
 * output is bit-identical whatever the batch, row or padded width.  steps = 0 gives mcg_shape_overlay's outputs bit for bit.
 * MCG_ERR_ARG, nothing launched: mcg_shape_overlay's argument errors, a null refine_ws / start_best / refined, steps
 * outside 0..1024, alpha not > 0. */
int mcg_shape_overlay_refined(const float* ref_frame, int n_ref, const float* ref_xform, const float* frames,
                              const float* xform, const int32_t* n_nodes_dev, int B, int N, const float* rot,
                              const float* axes, int n, float alpha, float amplitude, float* f_scratch, float* score,
                              float* best, int32_t* which, int32_t* flipped, float* pose, float* posed, int steps,
                              float* refine_ws, float* objective, float* start_best, int32_t* refined,
                              float* refined_score, void* stream);

/* ---- Pairwise shape Tanimoto ("shape diversity"): every pair of B molecules that already share
 * one frame (posed onto the reference by mcg_shape_overlay), compared as placed, with no orientation search.
 *   coords[B,N,3] with n_nodes_dev[b] real atoms (device memory, clamped to [0, N] on the device), in the reference's
 *   own coordinates; ref_xform[12] = the reference's M_r row-major, then t_r (mcg_shape_frames_tf), which maps every
 *   molecule into the reference's frame, y = (x - t_r) @ M_r; axes[3,n] = the reference frame's grid (atoms off the grid
 *   are cut off).  density_ws[B * Gp] with Gp = n^3 rounded up to a multiple of MCG_SHAPE_PAIR_KALIGN: the densities
 *   F (as mcg_shape_tanimoto evaluates them); gram_ws[B * B]: G = F F^T (exact fp32 MFMA); tanimoto[B * B], row-major:
 *   T_ij = G_ij / (G_ii + G_jj - G_ij).  T is exactly symmetric, T_ii is exactly 1 where the density is finite and not
 *   zero, and T_ij depends only on molecules i and j and the reference: the k order of every sum is fixed by n alone, so
 *   an entry has the same bits whatever the batch, row order or padded width.  A molecule with no atoms or a non-finite
 *   coordinate has a NaN density and so a NaN row and column; the other entries are unaffected.
 * MCG_ERR_ARG, nothing launched: a null buffer, B outside 1..MCG_SHAPE_PAIR_MAX_B, N outside 1..64, n outside
 * 2..MCG_SHAPE_PAIR_MAX_N. */
#define MCG_SHAPE_PAIR_MAX_B 16384
#define MCG_SHAPE_PAIR_MAX_N 256
#define MCG_SHAPE_PAIR_KALIGN 128
int mcg_shape_pair_tanimoto(const float* coords, const int32_t* n_nodes_dev, int B, int N, const float* ref_xform,
                            const float* axes, int n, float alpha, float amplitude, float* density_ws, float* gram_ws,
                            float* tanimoto, void* stream);

/* ---- Receptor contacts ("Receptor clashes"): the steric overlap of every ligand heavy atom with a
 * receptor, by brute force over all receptor atoms.
 *   lig_xyz[B,N,3] with n_nodes_dev[b] real atoms (device memory, clamped to [0, N] on the device), lig_radius[B,N] their
 *   van der Waals radii; rec_xyz[R,3], rec_radius[R] the receptor's heavy atoms (finite: the caller's check).
 *   overlap_out[B,N]: max_j (r_i + r_j) - sqrt(dx*dx + dy*dy + dz*dz), d = x_i - y_j, in fp32 in exactly that order
 *   (no contraction, correctly rounded sqrt); -inf on padded atoms; NaN for an atom with a non-finite coordinate (the
 *   other atoms are unaffected).
 *   splits: the receptor is cut into min(splits, ceil(R / 256)) ranges walked by different workgroups, their maxima
 *   combined by a second launch in partial_ws[splits * B * N] (not read, and may be NULL, when splits = 1).  A maximum is
 *   exact, so every output has the same bits whatever the splits, batch, row, padded width or receptor atom order.
 * MCG_ERR_ARG (1, the value of hipErrorInvalidValue), nothing launched: a null buffer, B outside 1..MCG_RECEPTOR_MAX_B,
 * N outside 1..64, R outside 1..MCG_RECEPTOR_MAX_ATOMS, splits outside 1..MCG_RECEPTOR_MAX_SPLITS, or splits > 1 without
 * partial_ws.
 * MCG_RECEPTOR_MAX_ATOMS is 512 tiles of 256 atoms: two full rounds of the tile list's compaction (csrc/mcg_receptor_tiles.h).
 * The limit itself, 65 536, 65 537 and 68 900 atoms are exercised by tests/test_large_receptor_gpu.py on all six receptor
 * entries. */
#define MCG_RECEPTOR_MAX_B 16384
#define MCG_RECEPTOR_MAX_ATOMS 131072
#define MCG_RECEPTOR_MAX_SPLITS 256
int mcg_receptor_overlap(const float* lig_xyz, const float* lig_radius, const int32_t* n_nodes_dev, int B, int N,
                         const float* rec_xyz, const float* rec_radius, int R, int splits, float* partial_ws,
                         float* overlap_out, void* stream);

/* ---- Clash relief ("Clash relief"): every posed molecule moved as a rigid body out of its steric
 * contacts with the receptor, one 256-lane workgroup per molecule, by a downhill accept / reject walk.
 *   lig_xyz[B,N,3], lig_radius[B,N], n_nodes_dev[B]: as for mcg_receptor_overlap.  rec_xyzr[R,4]: the receptor's heavy
 *   atoms as (x, y, z, van der Waals radius), 16-byte aligned, finite (the caller's check).
 *   Contact depth h_ij = max(0, ((r_i + r_j) - margin) - |x_i - y_j|); penalty P = sum h_ij^2; force on atom i
 *   F_i = sum_j 2 h_ij (x_i - y_j) / |x_i - y_j| (0 at distance 0); torque about the ligand's atom centroid.  Motion
 *   x' = (x - c) @ G + p, c the input's atom centroid, from G = I, p = c.  A trial rotates by s_r about the torque and
 *   moves by s_t along the net force (from 0.05 rad, 0.25 A) and is kept only if P strictly decreases (both lengths x 1.2,
 *   else x 0.5); a trial with |p - c| > max_shift is rejected the same way; `steps` trials, ended early only by P == 0.
 *   G is re-orthonormalised as each trial is formed, so the returned pose is the one that was evaluated.
 *   tile_sphere[ceil(R / 256), 4] or NULL: centre and radius of each tile of 256 consecutive receptor atoms, the radius
 *   including the tile's largest atom radius.  A workgroup then walks only the tiles within reach of its molecule; pairs
 *   out of contact are never summed, so the outputs have the same bits with and without it.
 *   coords_out[B,N,3]: the moved rows (padded rows zero); xform_out[B,12]: rotation row-major, then translation, with
 *   x' = x @ R + t; stats_out[B,4]: P before, P after, accepted steps, heavy-atom RMSD between input and output;
 *   gradient_out[B,6] (may be NULL): net force and torque at the start.  A molecule no step of which was accepted (P = 0
 *   at the start included) returns its input rows bit for bit, R = I, t = 0.  A molecule without atoms or with a
 *   non-finite coordinate returns its rows as they came and NaN in xform, stats and gradient; the others are unaffected.
 *   Every output depends on the molecule's own atoms and the receptor array only: the same bits in any batch, row, width.
 * MCG_ERR_ARG, nothing launched: a null buffer (tile_sphere and gradient_out excepted), B outside 1..MCG_RECEPTOR_MAX_B,
 * N outside 1..64, R outside 1..MCG_RECEPTOR_MAX_ATOMS, steps outside 0..1024, margin or max_shift negative or not
 * finite. */
int mcg_receptor_relieve(const float* lig_xyz, const float* lig_radius, const int32_t* n_nodes_dev, int B, int N,
                         const float* rec_xyzr, int R, const float* tile_sphere, int steps, float margin,
                         float max_shift, float* coords_out, float* xform_out, float* stats_out, float* gradient_out,
                         void* stream);

/* ---- Chemical fingerprints ("Chemical fingerprints"): a circular, Morgan-type fingerprint (radius
 * 2, 2 048 bits, bond types on, chirality off) and a graph identity key of B molecular graphs.  The definition is this
 * package's own (DESIGN.md states it in full): a SUBSTITUTE for RDKit's Morgan fingerprint, not bit-compatible with it.
 *   mcg_graph_fingerprint: z[B,W] atomic numbers, bonds[B,W,W] symmetric bond codes (0 none / 1 / 2 / 3 / 4 aromatic;
 *                          any other value is no bond), n_nodes_dev[b] real atoms (device memory, clamped to [0, W] on
 *                          the device; the diagonal and everything at or beyond n_b is ignored, whatever it holds).
 *                          fp_out[B, MCG_FP_WORDS]: bit k in word k >> 5 at position k & 31; key_out[B]: the 64-bit graph
 *                          key - equal for isomorphic graphs
 *                          (the converse can fail: graphs colour refinement cannot tell apart, or a hash collision);
 *                          popcount_out[B] (optional, NULL = not wanted): the set bits.  One 64-lane workgroup per
 *                          molecule; integer arithmetic only, so every output has the same bits whatever the batch, the
 *                          row and the padded width, and fingerprint and key do not depend on the atom numbering.
 *   mcg_fingerprint_tanimoto:      out[b] = T(fp[b], ref_fp), ref_fp[MCG_FP_WORDS].
 *   mcg_fingerprint_pair_tanimoto: out[B,B], row-major: T(fp[i], fp[j]); exactly symmetric, diagonal exactly 1.
 *   T(A, B) = float(c) / float(u), c = popcount(A & B), u = popcount(A | B), one correctly rounded fp32 division; NaN
 *   where A or B has no bit set (a molecule without atoms: its whole row and column), the other entries unaffected.
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null required buffer, B < 0, W outside 1..64, B above
 * MCG_SHAPE_PAIR_MAX_B (pair matrix). */
#define MCG_FP_WORDS 64
int mcg_graph_fingerprint(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                          uint32_t* fp_out, uint64_t* key_out, int32_t* popcount_out, void* stream);
int mcg_fingerprint_tanimoto(const uint32_t* fp, const uint32_t* ref_fp, int B, float* out, void* stream);
int mcg_fingerprint_pair_tanimoto(const uint32_t* fp, int B, float* out, void* stream);

/* ---- Solid references ("Solid references"): a watertight triangle mesh as the reference shape.
 * tri[F,9] = the corners a, b, c of every face (outward normals: counter-clockwise seen from outside), device memory.
 *   w(p) = (1 / 4 pi) sum_f 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|),  a, b, c = corner - p
 * the generalized winding number: +1 inside a closed outward mesh, 0 outside; an open mesh is a legal input.  fp32, one
 * lane per point, the triangles staged in tiles of 256.  The triangle range is cut into mcg_mesh_splits(F) parts (a
 * function of F alone: 4 tiles per part, at most 64 parts) walked by different workgroups, their sums added in part order
 * by a second launch through partial_ws[mcg_mesh_splits(F) * P] (not read, and may be NULL, when there is one part).
 * Every sum has one order, so w of a point has the same bits whatever P, its place among the points, array or grid
 * mode, and in mcg_mesh_atoms_outside.  A point on a corner of the mesh contributes atan2(0, 0) = 0, not NaN; the value
 * at a point exactly ON the surface is unspecified.  A non-finite point gets NaN, the other points are unaffected.
 *   mcg_mesh_winding:   w_out[P] of points[P,3], or - points NULL - w_out[n^3] of the grid points of axes[3,n] in
 *                       meshgrid(indexing="ij") flatten order (the grid of the shape kernels).  Exactly one of points / axes.
 *   mcg_mesh_occupancy: grid mode, writing f_out[idx] = |w| > 0.5 ? 1 : 0 - the density of the solid, for
 *                       mcg_shape_tanimoto_field / mcg_shape_overlay_field.  The indicator function as the density of a solid
 *                       is this package's own choice (the reference scores molecules against molecules only).
 *   mcg_mesh_atoms_outside: posed[B,N,3] with n_nodes_dev[b] real atoms (clamped to [0, N] on the device): outside[b] = the
 *                       real atoms with |w| <= 0.5, or -1 for a row with a non-finite real coordinate; w_out[B,N] (optional,
 *                       NULL = not wanted): the atoms' winding numbers, 0 on padded atoms.  One launch, one 64-lane
 *                       workgroup per row, no work space.
 *   mcg_shape_tanimoto_field / mcg_shape_overlay_field: mcg_shape_tanimoto / mcg_shape_overlay with the density launch
 *                       skipped and f[n^3] supplied by the caller: the same kernels, outputs and failure rows; with f = what
 *                       the density launch would have written (their f_scratch), the same bits.
 * MCG_ERR_ARG, nothing launched: a null required buffer, F outside 1..MCG_MESH_MAX_FACES, P outside 1..MCG_MESH_MAX_POINTS,
 * n outside 2..MCG_MESH_MAX_N, both or neither of points / axes, partial_ws NULL when mcg_mesh_splits(F) > 1, B < 1,
 * N outside 1..64 (atoms_outside, overlay_field, tanimoto_field; B * 64 <= MCG_MESH_MAX_POINTS), R < 1 (tanimoto_field).
 * mcg_mesh_splits returns 0 for an F outside the range. */
#define MCG_MESH_MAX_FACES 1048576
#define MCG_MESH_MAX_POINTS 16777216
#define MCG_MESH_MAX_N 256
int mcg_mesh_splits(int F);
int mcg_mesh_winding(const float* tri, int F, const float* points, int P, const float* axes, int n, float* w_out,
                     float* partial_ws, void* stream);
int mcg_mesh_occupancy(const float* tri, int F, const float* axes, int n, float* f_out, float* partial_ws, void* stream);
int mcg_mesh_atoms_outside(const float* tri, int F, const float* posed, const int32_t* n_nodes_dev, int B, int N,
                           int32_t* outside, float* w_out, void* stream);
int mcg_shape_tanimoto_field(const float* f, const float* cand, const int32_t* n_nodes_dev, int B, int N, const float* rot,
                             int R, const float* axes, int n, float alpha, float amplitude, float* score, void* stream);
int mcg_shape_overlay_field(const float* f, const float* ref_xform, const float* frames, const float* xform,
                            const int32_t* n_nodes_dev, int B, int N, const float* rot, const float* axes, int n,
                            float alpha, float amplitude, float* score, float* best, int32_t* which, int32_t* flipped,
                            float* pose, float* posed, void* stream);

/* ---- Relaxed geometry ("Relaxed geometry"): the heavy atoms of B molecules moved downhill on a
 * small restrained valence force field.  The force field is this package's OWN (DESIGN.md states it in full): a SUBSTITUTE
 * for the reference's MMFF94 clean-up, NOT MMFF94 - harmonic bond, 1-3 distance and one-sided non-bonded terms plus the
 * reference's position restraint (flat to 0.2 A, then 800 kcal/mol/A^2); no torsions, impropers, charges or hydrogens.
 *   coords[B,N,3] the start coordinates; z[B,W] atomic numbers, bonds[B,W,W] symmetric bond codes (0 none / 1 / 2 / 3 /
 *   4 aromatic; the diagonal, other codes and everything at or beyond n_b are read as 0), n_nodes_dev[b] real atoms
 *   (device memory, clamped to [0, min(W, N)] on the device).  N and W are independent: N is the row width of the
 *   coordinate buffers, W that of z and bonds.
 *   steps trial steps of x' = x - (s / max_i |g_i|) g from s = 0.02 A: accepted only if E(x') < E(x) (then s *= 1.2, else
 *   s *= 0.5); it stops early only where max_i |g_i| == 0.  steps = 0 copies the real atoms' coordinates bit for bit.
 *   coords_out[B,N,3] (zero on padded atoms; may not alias coords); energy_out[B,2] = E at the start, E at the end;
 *   grad_out[B,N,3] (optional, NULL = not wanted): dE/dx at the START coordinates, zero on padded atoms; stats_out[B,2]
 *   (optional): accepted steps, largest distance of an atom from where it started.  n = 0 and n = 1 change nothing and
 *   have E = 0.  A row with an element the library has no covalent radius for is copied unchanged with NaN energies (the
 *   Python layer refuses it before the launch).
 *   mcg_geometry_relax_ex: the same with restraint_ref[B,N,3] (optional, NULL = coords) as the positions the restraint
 *   holds every atom to - a relaxation continued from moved coordinates stays restrained to the original ones.
 * One 64-lane workgroup per molecule, no atomics, every sum in one order: a molecule's outputs have the same bits whatever
 * the batch, its row and the two padded widths.
 * MCG_ERR_ARG, nothing launched: a null required buffer, B < 0, N < 1, W outside 1..MCG_RELAX_MAX_ATOMS, steps outside
 * 0..MCG_RELAX_MAX_STEPS.  B = 0 launches nothing. */
#define MCG_RELAX_MAX_ATOMS 64
#define MCG_RELAX_MAX_STEPS 4096
int mcg_geometry_relax(const float* coords, const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                       int B, int N /*coords row width*/, int W /*z, bonds width*/, int steps,
                       float* coords_out, float* energy_out /*[B,2] start, end*/,
                       float* grad_out /*optional [B,N,3]: gradient at the START coordinates*/,
                       float* stats_out /*optional [B,2]: accepted steps, max atom displacement*/, void* stream);
int mcg_geometry_relax_ex(const float* coords, const float* restraint_ref, const int32_t* z, const int8_t* bonds,
                          const int32_t* n_nodes_dev, int B, int N, int W, int steps, float* coords_out,
                          float* energy_out, float* grad_out, float* stats_out, void* stream);

/* ---- Pharmacophore overlap ("Pharmacophore overlap"): the typed interaction features of B molecular
 * graphs and the Gaussian overlap of their posed features with a reference's.  The definition is this package's OWN
 * (DESIGN.md states it in full): not RDKit's feature factory, not a vendor's colour force field.  Types: donor, acceptor,
 * cation, anion, hydrophobe (per-atom bits 1, 2, 4, 8, 16; type indices 0..4) and ring (index 5: one feature per aromatic
 * ring of 5 or 6, at the fp32 centroid of its members).  No aromaticity is perceived: a ring counts where its bonds
 * carry code 4.
 *   mcg_pharm_perceive: z[B,W] atomic numbers, bonds[B,W,W] symmetric bond codes (1 / 2 / 3 / 4 aromatic; any other value
 *                       is no bond), n_nodes_dev[b] real atoms (device memory, clamped to [0, W] on the device; the
 *                       diagonal and everything at or beyond n_b is ignored, whatever it holds).  types_out[B,W]: the
 *                       per-atom type bits, 0 on padded atoms; n_rings_out[b]: the molecule's aromatic rings, the TRUE
 *                       count; ring_mask_out[B, MCG_PHARM_MAX_RINGS]: the member masks (bit k = atom k) of the first
 *                       MCG_PHARM_MAX_RINGS rings in ascending order of the mask read as an unsigned integer, 0 beyond the
 *                       count.  One 64-lane workgroup per molecule, integer arithmetic only: the same bits whatever the
 *                       batch, the row, the padded width and the padding's contents.
 *   mcg_pharm_score:    coords[B,N,3] (n_b clamped to [0, min(N, W)]), types[B,W], ring_mask[B, MCG_PHARM_MAX_RINGS] and
 *                       n_rings[B] as perceived; ref_xyz[F,3], ref_type[F] (type indices 0..5) the reference's features.
 *                       O(X, Y) = sum over equal-typed pairs of expf(-0.5 * d2), d2 = dx*dx + dy*dy + dz*dz in fp32 in
 *                       exactly that order (no contraction), the terms added in fp64 in one order fixed by the two feature
 *                       lists.  o_rm[b] = O(reference, molecule b), o_mm[b] = O(b, b), tanimoto[b] = o_rm / (o_rr + o_mm -
 *                       o_rm) rounded to fp32 with o_rr = *o_rr (device memory; NULL: the row's own o_mm), matches[b] = the
 *                       reference features with a feature of b of their type at d2 <= 2.25; per_type[B,6] (optional, NULL
 *                       = not wanted): the six parts of o_rm, which add up to it in type order.  A molecule without
 *                       features has tanimoto 0 and matches 0; one with a non-finite coordinate on a real atom or with
 *                       n_rings > MCG_PHARM_MAX_RINGS has NaN overlaps, a NaN tanimoto and matches -1, the other rows
 *                       unaffected.  coords NULL (B <= 1; n_nodes_dev, types, ring_mask, n_rings not read): the reference's
 *                       own list is the candidate - o_mm[0] of that run is O(R,R), by the same code.  One 64-lane
 *                       workgroup per molecule; every output has the same bits whatever the batch, the row and the widths.
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null required buffer, B < 0, W or N outside 1..64, F outside
 * 1..MCG_PHARM_MAX_FEATURES, coords NULL with B > 1. */
#define MCG_PHARM_MAX_RINGS 32
#define MCG_PHARM_MAX_FEATURES 352 /* 64 atoms x 5 atom types + MCG_PHARM_MAX_RINGS */
int mcg_pharm_perceive(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                       uint8_t* types_out, int32_t* n_rings_out, uint64_t* ring_mask_out, void* stream);
int mcg_pharm_score(const float* coords, const int32_t* n_nodes_dev, const uint8_t* types, const uint64_t* ring_mask,
                    const int32_t* n_rings, int B, int N /*coords row width*/, int W /*types width*/,
                    const float* ref_xyz, const uint8_t* ref_type, int F, const double* o_rr /*optional*/, double* o_rm,
                    double* o_mm, float* tanimoto, int32_t* matches, double* per_type /*optional [B,6]*/, void* stream);

/* ---- Explicit hydrogens ("Explicit hydrogens"): how many hydrogens each heavy atom of B molecular
 * graphs carries and where they sit.  The definition is this package's OWN (DESIGN.md states it in full): not RDKit's
 * AddHs - no charges, no protonation states, no tautomer search.  The count is the pharmacophore perception's nH plus one
 * aromatic N-H per aromatic 5-ring; a parent is linear, planar (conjugated N and O included) or tetrahedral by its bond
 * codes; X-H = rcov(Z) + 0.31 A along ideal directions; a parent with one neighbour is a rotor whose torsion is the one of
 * 12 (planar: 2) candidates that keeps its hydrogens clear of the other atoms.
 *   mcg_hydrogens_place: coords[B,N,3] fp32 heavy-atom coordinates, z[B,W] atomic numbers, bonds[B,W,W] symmetric bond
 *                       codes (1 / 2 / 3 / 4 aromatic; any other value is no bond), n_nodes_dev[b] real atoms (device
 *                       memory, clamped to [0, min(N, W)] on the device; the diagonal and everything at or beyond n_b is
 *                       ignored, whatever it holds); types[B,W], ring_mask[B, MCG_PHARM_MAX_RINGS] and n_rings[B] as
 *                       mcg_pharm_perceive wrote them for the same z, bonds and n_nodes (passed in, not perceived again).
 *                       h_xyz_out[B,HW,3]: the hydrogens in ascending order of the parent, then of m, zero beyond the
 *                       row's count; h_parent_out[B,HW]: each hydrogen's heavy atom, -1 beyond the count;
 *                       h_count_out[B,W]: the hydrogens placed on each heavy atom; n_h_out[b]: the row's count;
 *                       unplaced_out[b]: the hydrogens the count rule gives atoms in a situation the definition places
 *                       none for; rotor_delta_out[B,W] (optional, NULL = not wanted): the chosen torsion offset in
 *                       degrees, -1 for an atom that is no rotor.  HW >= max(4, 3 W): an atom with a neighbour carries at
 *                       most 3 hydrogens, a one-atom molecule at most 4 (an atom without a neighbour in a larger molecule
 *                       gets none: they count as unplaced).  A row with a non-finite coordinate on a real atom has
 *                       n_h = -1 and no hydrogens, the other rows unaffected.  A Z without a covalent radius is read with
 *                       radius 0 (the Python layer refuses it before the launch).  One 64-lane workgroup per molecule,
 *                       one launch, no atomics, fp32 with every product and sum rounded on its own and in one order: a
 *                       molecule's outputs have the same bits whatever the batch, its row and the padded widths.
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null required buffer, B outside 0..MCG_HYDROGENS_MAX_B, N < 1,
 * W outside 1..MCG_HYDROGENS_MAX_ATOMS, HW < max(4, 3 W). */
#define MCG_HYDROGENS_MAX_ATOMS 64
#define MCG_HYDROGENS_MAX_B 16384
int mcg_hydrogens_place(const float* coords, const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                        const uint8_t* types, const uint64_t* ring_mask, const int32_t* n_rings, int B,
                        int N /*coords row width*/, int W /*z, bonds, types width*/, int HW /*hydrogen slots per row*/,
                        float* h_xyz_out, int32_t* h_parent_out, int32_t* h_count_out, int32_t* n_h_out,
                        int32_t* unplaced_out, int32_t* rotor_delta_out /*optional [B,W]*/, void* stream);

/* ---- Standardised graphs ("Standardised graphs"): the largest fragment of each of B molecular
 * graphs, the checks that make it a molecule, and a Kekule form of its aromatic bonds.  The definition is this package's
 * OWN (DESIGN.md states it in full): not RDKit's FragmentParent / Kekulize / SanitizeMol - no charges, no normalisation,
 * no agreement with RDKit claimed.
 *   mcg_standardize_graphs: coords[B,N,3] fp32, z[B,W] atomic numbers, bonds[B,W,W] symmetric bond codes (1 / 2 / 3 / 4
 *                       aromatic; any other value is no bond; the matrix is read through its lower triangle),
 *                       n_nodes_dev[b] real atoms (device memory, clamped to [0, min(N, W)] on the device; the diagonal
 *                       and everything at or beyond n_b is ignored, whatever it holds).
 *                       The parent is the connected component with the most atoms, ties to the larger sum of atomic
 *                       numbers, then to the one holding the lowest atom index; its atoms keep their relative order.
 *                       coords_out[B,N,3] (copied bit for bit), z_out[B,W], bonds_out[B,W,W]: the parent, compacted, zero
 *                       beyond its atoms; atom_map_out[B,W]: the old index of each new atom, -1 beyond; n_out[b],
 *                       n_fragments_out[b], atoms_removed_out[b]; status_out[b]: 0 = valid, else a set of
 *                       MCG_STANDARDIZE_EMPTY (n = 0), _OVER_VALENCE (a kept atom's bonds, codes 1/2/3/4 counting
 *                       2/4/6/2 half-bonds, exceed twice the validity proxy's maximum valence), _AROMATIC_BRIDGE (a code-4
 *                       bond in no ring), _NOT_KEKULIZABLE and _SEARCH_BUDGET (the Kekule search of DESIGN.md failed, or
 *                       took more than MCG_STANDARDIZE_KEKULE_BUDGET steps on one component of the eligible graph; the
 *                       search runs only when the first three are clear).  kekule_out[B,W,W]: the parent's codes with
 *                       every code 4 replaced by 2 on the matched pairs and by 1 elsewhere; all zero unless status is 0.
 *                       The coordinates play no part in the verdict.  One 64-lane workgroup per molecule, one launch, no
 *                       atomics, integer work only: a molecule's outputs have the same bits whatever the batch, its row
 *                       and the padded widths.
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null buffer, B outside 0..MCG_STANDARDIZE_MAX_B, N < 1,
 * W outside 1..MCG_STANDARDIZE_MAX_ATOMS. */
#define MCG_STANDARDIZE_MAX_ATOMS 64
#define MCG_STANDARDIZE_MAX_B 16384
#define MCG_STANDARDIZE_KEKULE_BUDGET 16384
#define MCG_STANDARDIZE_EMPTY 1
#define MCG_STANDARDIZE_OVER_VALENCE 2
#define MCG_STANDARDIZE_AROMATIC_BRIDGE 4
#define MCG_STANDARDIZE_NOT_KEKULIZABLE 8
#define MCG_STANDARDIZE_SEARCH_BUDGET 16
int mcg_standardize_graphs(const float* coords, const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B,
                           int N /*coords row width*/, int W /*z, bonds width*/, float* coords_out, int32_t* z_out,
                           int8_t* bonds_out, int8_t* kekule_out, int32_t* atom_map_out, int32_t* n_out,
                           int32_t* n_fragments_out, int32_t* atoms_removed_out, int32_t* status_out, void* stream);

/* ---- Electrostatic similarity ("Electrostatic similarity"): partial charges of B molecular graphs by
 * iterative electronegativity equalisation (PEOE) and the Tanimoto of the Coulomb overlap of Gaussian-smeared point
 * charges with a reference's.  The definition is this package's OWN (DESIGN.md states it in full): not RDKit's
 * ComputeGasteigerCharges, not a vendor's electrostatic score - no formal charges, no protonation states.
 *   mcg_charges_peoe:   z[B,W] atomic numbers, bonds[B,W,W] symmetric bond codes (1 / 2 / 3 / 4 aromatic; any other value
 *                       is no bond), n_nodes_dev[b] real atoms (device memory, clamped to [0, W] on the device; the
 *                       diagonal and everything at or beyond n_b is ignored, whatever it holds); types[B,W],
 *                       ring_mask[B, MCG_PHARM_MAX_RINGS] and n_rings[B] as mcg_pharm_perceive wrote them for the same z,
 *                       bonds and n_nodes.  Per heavy atom nH and the class linear / planar / tetrahedral are those of
 *                       mcg_hydrogens_place; chi(q) = a + b q + c q^2 with the Gasteiger-Marsili (a, b, c) of the element
 *                       and class (H, C, N, O, F, P, S, Cl, Br), chi+ = a + b + c (H: 20.02); all charges start at 0;
 *                       steps k = 1..6, each from the charges of the step before: an atom adds, in fp32 and in ascending
 *                       neighbour index, f_ij = (chi_j - chi_i) / (chi+_i if chi_j > chi_i else chi+_j) over its bonded
 *                       atoms (any code once), then nH f_iH for its hydrogens, which share one charge that moves by
 *                       -f_iH; every update is multiplied by 0.5^k.  q_out[B,W]: the heavy atoms' charges;
 *                       qh_out[B,W]: the charge of EACH hydrogen of that atom, 0 where nH = 0; nh_out[B,W]: nH;
 *                       status_out[b]: 0, or 1 for a row with a real atom of an element without parameters - its real
 *                       atoms get NaN in q_out and qh_out, the other rows are unaffected.  Every element of every output
 *                       is written: 0 at and beyond a row's atoms.  One 64-lane wave per molecule, four molecules per
 *                       workgroup, no atomics, no scratch; products and sums rounded one by one in one order: a row's
 *                       outputs have the same bits whatever the batch, its row and the padded width.
 *   mcg_esp_overlap:    ref_xyz[P,3], ref_q[P] the reference's charge points; xyz[B,PW,3], q[B,PW] the candidates',
 *                       n_points[b] real points (device memory, clamped to [0, PW]).  E(X, Y) = sum_i sum_j qx_i qy_j
 *                       K(|x_i - y_j|), K(r) = erff(mu r) / r, below r = 1e-3: mu (2 / sqrt pi) (1 - (mu r)^2 / 3), r =
 *                       sqrtf(dx*dx + dy*dy + dz*dz) in fp32 in exactly that order (no contraction); a term is (qx_i *
 *                       qy_j) * K in fp32; thread t of the row's 256 adds the terms of candidate point t in fp64 in
 *                       ascending j, the threads' sums are added in fp64 by one binary tree (t takes t + 128, + 64, ...
 *                       + 1) and rounded to fp32 once.  cross[b] = E(reference, b), self[b] = E(b, b) (i = j included),
 *                       tanimoto[b] = cross / ((e_rr + self) - cross) in fp32 with e_rr = *e_rr (device memory; NULL: the
 *                       row's own self), 0 where that denominator is below 1e-12.  A row with a non-finite coordinate or
 *                       charge on a real point has NaN in all three, the other rows unaffected.  The reference run as its
 *                       own one-row batch gives E(R,R) as self[0], by the same code.  One 256-thread workgroup per row; a
 *                       row's outputs have the same bits whatever the batch, its row and PW.
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null required buffer, B outside 0..MCG_CHARGES_MAX_B /
 * 0..MCG_ESP_MAX_B, W outside 1..MCG_CHARGES_MAX_ATOMS, P or PW outside 1..MCG_ESP_MAX_POINTS, mu not positive and finite. */
#define MCG_CHARGES_MAX_ATOMS 64
#define MCG_CHARGES_MAX_B 16384
#define MCG_ESP_MAX_POINTS 256 /* 64 heavy atoms + 3 x 64 hydrogens */
#define MCG_ESP_MAX_B 16384
int mcg_charges_peoe(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, const uint8_t* types,
                     const uint64_t* ring_mask, const int32_t* n_rings, int B, int W /*z, bonds, types width*/,
                     float* q_out, float* qh_out, int32_t* nh_out, int32_t* status_out, void* stream);
int mcg_esp_overlap(const float* ref_xyz, const float* ref_q, int P, const float* xyz, const float* q,
                    const int32_t* n_points, int B, int PW /*points per row*/, float mu, const float* e_rr /*optional*/,
                    float* cross_out, float* self_out, float* tanimoto_out, void* stream);

/* ---- Canonical graphs ("Canonical graphs and SMILES"): an exact canonical atom order of each of B
 * molecular graphs.  The definition is this package's OWN (DESIGN.md states it in full): not RDKit's canonical ranking, no
 * agreement with any toolkit claimed.
 *   mcg_canonical_order: z[B,W] atomic numbers, bonds[B,W,W] symmetric bond codes (1 / 2 / 3 / 4 aromatic; any other
 *                       value is no bond), n_nodes_dev[b] real atoms (device memory, clamped to [0, W] on the device; the
 *                       diagonal and everything at or beyond n_b is ignored, whatever it holds).
 *                       Initial colour (Z, degree, twice the bond-order sum with aromatic 1.5); rank = the number of atoms
 *                       with a smaller key, tied atoms share a rank (a cell).  Refinement: key = (rank, the neighbours'
 *                       (rank, code) pairs ascending), ranked again, until no cell splits.  Search: the target cell is the
 *                       non-singleton cell of smallest rank r; for each member v in ascending index - skipping one that
 *                       has a twin (same Z, same code to every third atom) among the members in front of it - v keeps r,
 *                       the other members get r + 1, refine, recurse.  A leaf (all cells singletons) gives order[k] = the
 *                       atom of rank k and the certificate Z(order[0..n-1]), then code(order[i], order[j]) for i = 1..n-1,
 *                       j = 0..i-1; the lexicographically smallest certificate wins, the first such leaf on ties.  At most
 *                       MCG_CANONICAL_LEAF_BUDGET leaves are visited.
 *                       order_out[B,W]: the canonical order, -1 beyond n_b; status_out[b]: 0, or MCG_CANONICAL_EMPTY (n =
 *                       0), _DEGREE (an atom with more than MCG_CANONICAL_MAX_DEGREE neighbours; nothing is searched) or
 *                       _BUDGET (a branch was still unexplored behind the last leaf allowed): such a row has -1 throughout
 *                       order_out and key 0; leaves_out[b]: the leaves visited; key_out[b]: 64 bits of the winning
 *                       certificate (MurmurHash3 under the fingerprint's two seeds) - for grouping, never for a decision.
 *                       One 64-lane workgroup per molecule, one launch, integer work only, no atomics, no scratch: a
 *                       molecule's outputs have the same bits whatever the batch, its row and the padded width, and
 *                       certificate, key and leaves do not depend on the atom numbering.
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null buffer, B outside 0..MCG_CANONICAL_MAX_B, W outside
 * 1..MCG_CANONICAL_MAX_ATOMS. */
#define MCG_CANONICAL_MAX_ATOMS 64
#define MCG_CANONICAL_MAX_B 16384
#define MCG_CANONICAL_MAX_DEGREE 8
#define MCG_CANONICAL_LEAF_BUDGET 4096
#define MCG_CANONICAL_EMPTY 1
#define MCG_CANONICAL_DEGREE 2
#define MCG_CANONICAL_BUDGET 4
int mcg_canonical_order(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                        int32_t* order_out, int32_t* status_out, int32_t* leaves_out, uint64_t* key_out, void* stream);

/* ---- Stereo identity ("Stereo identity"): which stereoisomer each of B EMBEDDED molecular graphs
 * is.  The definition is this package's OWN (DESIGN.md states it in full): not RDKit's stereo perception, no CIP labels.
 *   mcg_stereo_order:   coords[B,W,3] fp32 heavy-atom coordinates (read for real atoms only: the padding may hold anything,
 *                       NaN included); z, bonds, n_nodes_dev, order_out, status_out, leaves_out, key_out as
 *                       mcg_canonical_order takes them, limits and status bits included.  Prepass: the tetrahedral
 *                       candidates (Z 6 / 14, single bonds only, heavy degree 4 or 3, no two terminal twins) with the sign
 *                       of the normalised signed volume of their neighbours in ascending index, and the double-bond
 *                       candidates (code 2 between Z 6 / 7, single bonds otherwise, one or two substituents per end, no two
 *                       terminal twins) with the signs of the dihedral cosines of their substituent pairs; |value| < 0.1,
 *                       a vanishing vector or inconsistent signs leave the candidate undefined.  Search: the canonical
 *                       search, except that a leaf whose certificate equals the best one wins if its stereo vector is
 *                       smaller, and that only twins of degree <= 1 are skipped.  The stereo vector of a leaf: v[k] = 4 tet +
 *                       db of the atom at position k; tet = 0, or 1 / 2 by sign x the parity that sorts the neighbours by
 *                       rank; db = 0, or 1 cis / 2 trans of the two lowest-ranked substituents, stored at the end of
 *                       larger rank.
 *                       stereo_out[B,W] int8: v in canonical position order, 0 beyond n_b and throughout a row whose status
 *                       is not 0; stereo_key_out[b]: the key's mixing over (n, row hashes, v) - for grouping, 0 where the
 *                       status is not 0; counts_out[B,3]: the defined tetrahedral descriptors, the defined double bonds,
 *                       the undefined candidates (of the prepass: whatever the status).  key_out equals
 *                       mcg_canonical_order's wherever both have status 0; leaves_out need not.
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null buffer, B outside 0..MCG_CANONICAL_MAX_B, W outside
 * 1..MCG_CANONICAL_MAX_ATOMS. */
int mcg_stereo_order(const float* coords, const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                     int32_t* order_out, int32_t* status_out, int32_t* leaves_out, uint64_t* key_out, int8_t* stereo_out,
                     uint64_t* stereo_key_out, int32_t* counts_out, void* stream);

/* ---- Substructure patterns ("Substructure patterns"): all embeddings of each of P query graphs in
 * each of B molecular graphs, exact in integers.  The definition is this package's OWN (DESIGN.md states it in full): a
 * small query language and a subgraph-monomorphism search, not RDKit's substructure matcher.
 *   mcg_substructure_match: z, bonds, n_nodes_dev as mcg_canonical_order takes them (no degree cap); nh_or_null[B,W]: the
 *                       hydrogens of every atom, or NULL: max(0, (2 v0 - v2) / 2) from the bond codes.
 *                       Pattern p, ALREADY IN MATCHING ORDER (per component breadth-first from its lowest atom, neighbours
 *                       ascending, components by their lowest atom - the host's business): pat_n[p] query atoms (clamped
 *                       to 0..32 on the device; 0 atoms match nothing);
 *                       pat_atoms[p][k] = two words: word 0 the element mask (bit Z set: allowed; all ones: any element,
 *                       also one beyond Z = 63), word 1 the bytes dmin, dmax, hmin, hmax, ring, arom from the low end
 *                       (dmin <= bonded atoms <= dmax, hmin <= hydrogens <= hmax; ring / arom: 0 any, 1 yes, 2 no - the
 *                       atom has a ring bond / a code-4 bond);
 *                       pat_bonds[p][k][q], read for q < k only: 0 no query bond, else the low nibble the allowed codes
 *                       (bit c - 1: code c) and bits 4-5 the ring requirement (0 any, 1 a ring bond, 2 a chain bond).  A
 *                       bond is a ring bond iff its ends stay connected without it.
 *                       An embedding is an injective map of the positions to atoms that satisfies every query atom and
 *                       lands every query bond on a bond that satisfies it; pairs without a query bond are free.  Search,
 *                       per root atom r ascending: position 0 takes r, position k then every atom, ascending, that is
 *                       unused, in k's domain and rightly bonded to the images of the earlier positions k has a query bond
 *                       with; each accepted assignment is a node; every embedding is enumerated.  A root that would take a
 *                       node beyond MCG_SUBSTRUCTURE_NODE_BUDGET stops there and the pair's status is _BUDGET.
 *                       count[b,p]: the embeddings found (a lower bound under _BUDGET); status[b,p]: 0 or _BUDGET;
 *                       first[b,p,0..31]: the atoms of the embedding found first (the smallest in matching order), -1
 *                       beyond the pattern's atoms and throughout where count is 0; covered[b,p]: bit a set where atom a
 *                       lies in any embedding found.
 *                       One 64-lane workgroup per (molecule, chunk of the patterns), lane = root atom, every lane its own
 *                       depth-first search on an LDS stack; one launch, integers only, no atomics, no scratch: a pair's
 *                       outputs have the same bits whatever the batch, the row, the padded width and the other patterns.
 * The pattern tables are device memory: any bytes in them are safe.  B = 0 launches nothing.  MCG_ERR_ARG, nothing
 * launched: a null buffer other than nh_or_null, B outside 0..MCG_SUBSTRUCTURE_MAX_B, W outside
 * 1..MCG_SUBSTRUCTURE_MAX_ATOMS, P outside 1..MCG_SUBSTRUCTURE_MAX_PATTERNS. */
#define MCG_SUBSTRUCTURE_MAX_ATOMS 64
#define MCG_SUBSTRUCTURE_MAX_PATTERN_ATOMS 32
#define MCG_SUBSTRUCTURE_MAX_PATTERNS 64
#define MCG_SUBSTRUCTURE_MAX_B 16384
#define MCG_SUBSTRUCTURE_NODE_BUDGET 65536
#define MCG_SUBSTRUCTURE_BUDGET 1
int mcg_substructure_match(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                           const int32_t* nh_or_null, int B, int W, const int32_t* pat_n,
                           const uint64_t* pat_atoms /*[P,32,2]*/, const uint8_t* pat_bonds /*[P,32,32]*/, int P,
                           int32_t* count /*[B,P]*/, int32_t* status /*[B,P]*/, int32_t* first /*[B,P,32]*/,
                           uint64_t* covered /*[B,P]*/, void* stream);

/* ---- Rings and scaffolds ("Rings and scaffolds"): general ring perception and the Murcko-type
 * scaffold of each of B molecular graphs, exact in integers.  The definitions are this package's OWN (DESIGN.md states them
 * in full): not RDKit's ring perception, not an SSSR, and NOT RDKit's MurckoScaffold.
 *   mcg_ring_scaffold:  z, bonds, n_nodes_dev as mcg_canonical_order takes them (no degree cap; z is not read: the
 *                       definitions are the graph's alone).
 *                       Ring bond: (a, j) iff j is reachable from a with that bond left out.  Ring atom: an atom with a
 *                       ring bond.  Ring system: a connected component of the ring-bond sub-graph (fused, bridged and
 *                       spiro rings are one system), labelled by its lowest atom.  Size of a ring bond: the shortest path
 *                       between its ends with the bond left out, plus 1; of an atom: the smallest over its ring bonds.
 *                       Linker atoms: remove, as long as one exists, every atom with fewer than two remaining neighbours;
 *                       the non-ring atoms that remain.  Exo atoms: atoms outside ring and linker joined to one of them by
 *                       a code-2 bond.  Scaffold = ring + linker + exo.
 *                       ring_nb_out[B,W]: bit j of entry a set iff (a, j) is a ring bond; 0 at and beyond n_b.
 *                       ring_size_out[B,W]: the atom's size, 0 for a non-ring atom and at and beyond n_b.
 *                       ring_system_out[B,W]: the atom's system label, -1 for a non-ring atom and at and beyond n_b.
 *                       masks_out[B,4]: bit a set iff atom a is a ring / linker / exo / scaffold atom, in this order.
 *                       counts_out[B,8]: n_rings = ring bonds - ring atoms + ring systems (the cyclomatic number),
 *                       n_ring_systems, min_ring_size, max_ring_size (the smallest and largest ring-bond size; 0, 0 for an
 *                       acyclic graph), ring atoms, linker atoms, exo atoms, ring bonds.
 *   mcg_induced_subgraph: z, bonds, n_nodes_dev likewise; mask[b]: bit a set keeps atom a (bits at and beyond n_b are
 *                       ignored); mode 0 keeps elements and bond codes (a value that is no code is written as 0), mode 1
 *                       writes Z = 6 and code 1 (the generic framework).  The kept atoms stay in ascending index,
 *                       compacted to the front: z_out[B,W], bonds_out[B,W,W] (zero behind the kept atoms, zero diagonal),
 *                       n_out[b] the kept atoms, map_out[B,W] the source index of each, -1 behind them.  The outputs are
 *                       padded graphs as mcg_canonical_order takes them, which gives a scaffold its identity.
 *                       Both: one 64-lane workgroup per molecule, one launch, integer work only, no atomics, no scratch:
 *                       a molecule's outputs have the same bits whatever the batch, its row and the padded width, and
 *                       counts, sizes and masks follow the atoms under any renumbering.
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null buffer, B outside 0..MCG_SCAFFOLD_MAX_B, W outside
 * 1..MCG_SCAFFOLD_MAX_ATOMS, a mode other than 0 or 1. */
#define MCG_SCAFFOLD_MAX_ATOMS 64
#define MCG_SCAFFOLD_MAX_B 16384
int mcg_ring_scaffold(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                      uint64_t* ring_nb_out /*[B,W]*/, int32_t* ring_size_out /*[B,W]*/,
                      int32_t* ring_system_out /*[B,W]*/, uint64_t* masks_out /*[B,4]*/, int32_t* counts_out /*[B,8]*/,
                      void* stream);
int mcg_induced_subgraph(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, const uint64_t* mask /*[B]*/,
                         int mode, int B, int W, int32_t* z_out /*[B,W]*/, int8_t* bonds_out /*[B,W,W]*/,
                         int32_t* n_out /*[B]*/, int32_t* map_out /*[B,W]*/, void* stream);

/* ---- Receptor interactions ("Receptor interactions"): an empirical interaction score of B posed
 * molecules against a typed receptor.  The definition is this package's OWN (interactions.py states it in full): the
 * functional form of the AutoDock Vina scoring function on the package's heavy-atom types, intermolecular terms only - NOT
 * AutoDock Vina's output and not a binding free energy.
 *   lig_xyz[B,N,3], lig_radius[B,N] (interaction radii), lig_type[B,N] (bits: 1 donor, 2 acceptor, 4 hydrophobic),
 *   n_nodes_dev[b] real atoms (device memory, clamped to [0, min(N, 64)] on the device; everything at or beyond n_b is
 *   ignored, whatever it holds), n_rot_dev[b] rotatable bonds (device memory, negative counts as 0);
 *   rec_xyzr[R,4] (x, y, z, interaction radius) and rec_type[R] (the same bits), in the order the caller wants them
 *   walked; tile_sphere: NULL, or [ceil(R / 256), 4] centre and radius of a sphere that holds every atom of each tile of
 *   256 consecutive receptor atoms - a tile whose sphere stays beyond the cut-off of the ligand's is skipped, which changes
 *   no bit.
 *   Pair (i, j): r2 = dx*dx + dy*dy + dz*dz in fp32, every operation rounded on its own in that order; the pair COUNTS iff
 *   r2 < 64.0f; d = sqrtf(r2) - (R_i + R_j).  Terms of a counted pair, all from the fp32 d: g1 = expf(-(2d)^2), g2 =
 *   expf(-((d - 3) / 2)^2), rep = d*d where d < 0, hyd (both hydrophobic) 1 at d <= 0.5, 1.5 - d up to 1.5, hb (a donor
 *   facing an acceptor, either way) 1 at d <= -0.7f, d / -0.7f up to 0; a pair that does not count adds nothing.
 *   atom_terms[B,N,6]: per atom the five sums over j and (((( -0.0356 g1 - 0.00516 g2) + 0.840 rep) - 0.0351 hyd) - 0.587
 *   hb); 0 on padded atoms.  mol_terms[B,8]: G1, G2, REP, HYD, HB, that weighted sum W of the five, E = W / (1 + 0.0585
 *   n_rot), 0.  hbonds[b]: the counted donor / acceptor pairs with d <= -0.7f, exact.
 *   A molecule without atoms: zeros.  One with a non-finite coordinate on a real atom: NaN in its real atoms' terms and in
 *   mol_terms[0..6], hbonds -1; the other rows unaffected.
 *   One 256-lane workgroup per molecule: lane l has atom l & 63, wave l >> 6 walks the receptor atoms j = wave (mod 4) of
 *   each kept tile in ascending order from LDS; an atom's four partial sums are added as (w0 + w1) + (w2 + w3), the
 *   molecule's by one butterfly over the 64 atom slots.  No atomics, no scratch: a molecule's outputs have the same bits
 *   whatever the batch, its row, the padded width and the tile skipping.
 * MCG_ERR_ARG, nothing launched: a null buffer (tile_sphere excepted), B outside 1..MCG_RECEPTOR_MAX_B, N outside 1..64,
 * R outside 1..MCG_RECEPTOR_MAX_ATOMS. */
int mcg_receptor_interactions(const float* lig_xyz, const float* lig_radius, const uint8_t* lig_type,
                              const int32_t* n_nodes_dev, const int32_t* n_rot_dev, int B, int N, const float* rec_xyzr,
                              const uint8_t* rec_type, int R, const float* tile_sphere /*optional*/,
                              float* atom_terms /*[B,N,6]*/, float* mol_terms /*[B,8]*/, int32_t* hbonds /*[B]*/,
                              void* stream);

/* ---- Optimised pose ("Optimised pose"): every posed molecule moved as a rigid body downhill on the
 * weighted sum W of the five interaction terms above (mol_terms[5]; E is W over a positive constant, so less W is less
 * E), one 256-lane workgroup per molecule, by the accept / reject walk of mcg_receptor_relieve.  The package's OWN
 * procedure: not a docking run, not AutoDock Vina's local optimisation; rigid body only - no torsions, no intramolecular
 * term, no hydrogens, no global search.
 *   lig_xyz, lig_radius, lig_type, n_nodes_dev, rec_xyzr, rec_type, tile_sphere: as for mcg_receptor_interactions; the
 *   pair arithmetic (r2, the r2 < 64.0f decision, d, the five terms), the lane layout and the order of every sum are that
 *   entry's, from one shared text, so W of a pose has the bits mol_terms[5] has for the same coordinates.
 *   Force on atom i: F_i = - sum_j (dW/dd) (x_i - y_j) / r over its counted pairs (direction 0 at r = 0), the slope decided
 *   on the same fp32 d as the terms: g1' = -8 d g1, g2' = -((d - 3) / 2) g2, rep' = 2 d where d < 0, hyd' = -1 on
 *   0.5 < d < 1.5 (both hydrophobic), hb' = 1 / -0.7f on -0.7f < d < 0 (donor facing acceptor), 0 elsewhere.
 *   Motion x' = (x - c) @ G + p, c the input's atom centroid summed in atom order, from G = I, p = c; the first evaluation
 *   reads the input rows as they came.  Torque about p: sum_i u_i x F_i, u_i = (x_i - c) @ G.  A trial rotates by s_r about
 *   the torque and moves p by s_t along the net force (from 0.05 rad, 0.25 A; a zero or non-finite vector skips its part
 *   of the move, both skipped ends the walk); a trial with |p' - c| > max_shift is rejected unevaluated; an evaluated one
 *   is kept iff W' < W strictly (NaN never is); kept: both lengths x 1.2, rejected: x 0.5.  The walk ends after `steps`
 *   trials or once s_t < 2^-8 A.  G is re-orthonormalised as each trial is formed, so the pose returned is the one scored.
 *   The tile list is built once, with max_shift added to the scoring entry's reach; it changes no bit.
 *   coords_out[B,N,3]: the kept pose (padded rows zero); xform_out[B,12]: rotation row-major, then translation, with
 *   x' = x @ R + t; stats_out[B,8]: W before, W after, trials used, trials kept, heavy-atom RMSD between input and output,
 *   the final s_t, 0, 0; gradient_out[B,6] (may be NULL): net force and torque at the input pose; trace_out[B,steps,24]
 *   (may be NULL; for tests): per trial F[3], torque[3] at the current pose, s_r, s_t, the trial's G'[9] and p'[3], W' (0
 *   where not evaluated), evaluated (0 / 1), kept (0 / 1), W of the current pose; rows beyond the last trial are zero.
 *   A molecule no trial of which was kept (steps = 0 and no counted pair included) returns its input rows bit for bit,
 *   R = I, t = 0.  A molecule without atoms or with a non-finite coordinate on a real atom returns its rows as they came
 *   and NaN in xform, stats and gradient (its trace rows zero); the others are unaffected.  Every output depends on the
 *   molecule's own atoms and the receptor arrays only: the same bits in any batch, row, width, with or without tile_sphere.
 * MCG_ERR_ARG, nothing launched: a null buffer (tile_sphere, gradient_out and trace_out excepted), B outside
 * 1..MCG_RECEPTOR_MAX_B, N outside 1..64, R outside 1..MCG_RECEPTOR_MAX_ATOMS, steps outside 0..1024, max_shift negative
 * or not finite. */
int mcg_receptor_optimise(const float* lig_xyz, const float* lig_radius, const uint8_t* lig_type,
                          const int32_t* n_nodes_dev, int B, int N, const float* rec_xyzr, const uint8_t* rec_type, int R,
                          const float* tile_sphere /*optional*/, int steps, float max_shift, float* coords_out /*[B,N,3]*/,
                          float* xform_out /*[B,12]*/, float* stats_out /*[B,8]*/, float* gradient_out /*optional [B,6]*/,
                          float* trace_out /*optional [B,steps,24]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MLCONFGEN_HIP_H */
