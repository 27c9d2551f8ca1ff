// Electrostatic similarity ("Electrostatic similarity"): partial charges of molecular graphs by
// iterative electronegativity equalisation (PEOE) and the Tanimoto of the Coulomb overlap of Gaussian-smeared charges.  The
// package's OWN definition - not RDKit's ComputeGasteigerCharges, not a vendor's electrostatic score: no formal charges, no
// protonation states.
//   k_charges_peoe: one 64-lane wave per molecule, lane = heavy atom, PE_MOLS molecules per workgroup.
//     stage   bond codes (68-byte rows) and the perceived ring masks -> the wave's slice of LDS.
//     rules   per lane the bond tally, nH and the class, by the code k_hydrogens_place runs (mcg_graph_rules.h); the
//             neighbours stay in a register as a 64-bit mask - the iteration reads no bond code again.
//     iterate six Jacobi steps: every lane writes its chi to LDS, a barrier, then walks its neighbour mask in ascending
//             index and adds f_ij, then nH f_iH for its own hydrogens; every update is multiplied by 0.5^k.
//     write   plain stores of q, q_h, nh (0 at and beyond the row's atoms; NaN charges in a row that holds an element
//             without parameters) and the row's status.
//   k_esp_overlap: one 256-thread workgroup per candidate row; the reference's and the row's points (x, y, z, q) in LDS.
//     Thread t owns candidate point t and walks the reference, then the row itself, in ascending index: fp32 terms, fp64
//     partial sums, then ONE binary tree over t (stride 128, 64, ... 1), the two sums rounded to fp32 once.
//   Products and sums are rounded one by one (no contraction), divisions and square roots are correctly rounded, and every
//   loop bound is the row's own count: a row's result has the same bits whatever the batch, its row and the padded widths.
//   No atomics, no inline assembly, no private arrays (no scratch), no global scratch.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_graph_rules.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int PE_MAXW = MCG_CHARGES_MAX_ATOMS;       // atoms per molecule: one lane and one mask bit each
constexpr int PE_MOLS = 4;                           // molecules (waves) per workgroup
constexpr int PE_STEPS = 6;
constexpr int PE_MAX_RINGS = MCG_PHARM_MAX_RINGS;
static_assert(PE_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");
constexpr float PE_H_A = 7.17f, PE_H_B = 6.24f, PE_H_C = -0.56f, PE_H_PLUS = 20.02f;

constexpr int ES_MAXP = MCG_ESP_MAX_POINTS;          // points per molecule: one thread each
constexpr float ES_SMALL_R = 1e-3f;
constexpr float ES_TWO_OVER_SQRT_PI = 1.1283791670955126f;
constexpr float ES_EMPTY = 1e-12f;

struct Abc {
    float a, b, c;
};

// chi(q) = a + b q + c q^2 of an atom of element z in class cls (mcg_graph_rules.h), the Gasteiger-Marsili values;
// `sulfone`: an S with two or more code-2 bonds to O.  false: no parameters for this element
__device__ __forceinline__ bool peoe_parameters(int z, int cls, bool sulfone, Abc& p) {
    const bool tet = cls == MCG_CLASS_TETRAHEDRAL, lin = cls == MCG_CLASS_LINEAR;
    switch (z) {
        case 1: p = Abc{PE_H_A, PE_H_B, PE_H_C}; return true;
        case 6: p = tet ? Abc{7.98f, 9.18f, 1.88f} : lin ? Abc{10.39f, 9.45f, 0.73f} : Abc{8.79f, 9.32f, 1.51f}; return true;
        case 7: p = tet ? Abc{11.54f, 10.82f, 1.36f} : lin ? Abc{15.68f, 11.70f, -0.27f} : Abc{12.87f, 11.15f, 0.85f}; return true;
        case 8: p = tet ? Abc{14.18f, 12.92f, 1.39f} : Abc{17.07f, 13.79f, 0.47f}; return true;
        case 9: p = Abc{14.66f, 13.85f, 2.31f}; return true;
        case 15: p = Abc{8.90f, 8.24f, 0.96f}; return true;
        case 16: p = sulfone ? Abc{12.00f, 10.81f, 1.20f} : tet ? Abc{10.14f, 9.13f, 1.38f} : Abc{10.88f, 9.49f, 1.33f}; return true;
        case 17: p = Abc{11.00f, 9.69f, 1.35f}; return true;
        case 35: p = Abc{10.08f, 8.47f, 1.16f}; return true;
        default: p = Abc{0.f, 0.f, 0.f}; return false;
    }
}

__device__ __forceinline__ float chi_of(const Abc& p, float q) { return (p.a + p.b * q) + p.c * (q * q); }

// the charge that flows onto atom i from atom j: (chi_j - chi_i) / chi+ of the one that gives electrons
__device__ __forceinline__ float flow(float chi_i, float plus_i, float chi_j, float plus_j) {
    return (chi_j - chi_i) / (chi_j > chi_i ? plus_i : plus_j);
}

__global__ __launch_bounds__(PE_MAXW * PE_MOLS) void k_charges_peoe(
    const int32_t* __restrict__ z, const int8_t* __restrict__ bonds, const int32_t* __restrict__ n_nodes,
    const uint8_t* __restrict__ types, const u64* __restrict__ ring_mask, const int32_t* __restrict__ n_rings, int B, int W,
    float* __restrict__ q_out, float* __restrict__ qh_out, int32_t* __restrict__ nh_out, int32_t* __restrict__ status_out) {
    __shared__ __attribute__((aligned(16))) uint8_t code_s[PE_MOLS][PE_MAXW * MCG_CODE_STRIDE];
    __shared__ u64 rings_s[PE_MOLS][PE_MAX_RINGS];
    __shared__ float chi_s[PE_MOLS][PE_MAXW], plus_s[PE_MOLS][PE_MAXW];
    __shared__ int32_t z_s[PE_MOLS][PE_MAXW];

    const int w = threadIdx.x / PE_MAXW, a = threadIdx.x % PE_MAXW;
    const int b = blockIdx.x * PE_MOLS + w;
    const bool row = b < B;                           // a wave beyond the batch keeps the barriers company and writes nothing
    const int n = row ? min(max(n_nodes[b], 0), W) : 0;
    const bool real = a < n;
    uint8_t* code = code_s[w];
    u64* rings = rings_s[w];

    if (row) mcg_stage_codes(code, bonds + (size_t)b * W * W, W, n, a, PE_MAXW);
    const u64 live = low_bits(n);
    const int nr = row ? min(max(n_rings[b], 0), PE_MAX_RINGS) : 0;
    if (a < PE_MAX_RINGS) rings[a] = a < nr ? (ring_mask[(size_t)b * PE_MAX_RINGS + a] & live) : 0ull;
    const int za = real ? z[(size_t)b * W + a] : 0;
    const int ta = real ? types[(size_t)b * W + a] : 0;
    z_s[w][a] = za;
    __syncthreads();

    const McgBondTally tally = mcg_bond_tally(code + a * MCG_CODE_STRIDE, real ? n : 0);
    const u64 m_has24 = __ballot(real && mcg_has_code_2_or_4(tally));
    const u64 m_ring_n = __ballot(real && mcg_ring_nh_candidate(za, tally, ta));
    const int cls = mcg_parent_class(za, tally, m_has24);
    const int nh = mcg_implicit_hydrogens(real, a, za, tally, rings, nr, m_ring_n);
    int oxo = 0;                                      // code-2 bonds to O
    for (u64 m = tally.m2; m != 0ull; m &= m - 1ull) oxo += z_s[w][low_bit(m)] == 8 ? 1 : 0;
    Abc p;
    const bool known = peoe_parameters(za, cls, za == 16 && oxo >= 2, p);
    const bool refused = __ballot(real && !known) != 0ull;
    const float plus = za == 1 ? PE_H_PLUS : (p.a + p.b) + p.c;
    const Abc ph = Abc{PE_H_A, PE_H_B, PE_H_C};
    plus_s[w][a] = plus;

    float q = 0.f, qh = 0.f, damp = 1.f;
    for (int k = 1; k <= PE_STEPS; ++k) {
        damp = damp * 0.5f;
        const float chi = chi_of(p, q);
        chi_s[w][a] = chi;
        __syncthreads();
        float s = 0.f;
        for (u64 m = tally.mask; m != 0ull; m &= m - 1ull) {      // ascending neighbour index
            const int j = low_bit(m);
            s = s + flow(chi, plus, chi_s[w][j], plus_s[w][j]);
        }
        if (nh > 0) {
            const float f = flow(chi, plus, chi_of(ph, qh), PE_H_PLUS);
            s = s + (float)nh * f;
            qh = qh - damp * f;
        }
        q = q + damp * s;
        __syncthreads();                              // every chi of this step is read before the next one is written
    }

    if (row && a < W) {
        const float nan = __int_as_float(0x7fc00000);
        const size_t at = (size_t)b * W + a;
        q_out[at] = real ? (refused ? nan : q) : 0.f;
        qh_out[at] = real ? (refused ? nan : (nh > 0 ? qh : 0.f)) : 0.f;
        nh_out[at] = nh;
    }
    if (row && a == 0) status_out[b] = refused ? 1 : 0;
}

// K(r) = erf(mu r) / r, the Coulomb kernel between two unit Gaussian charges; its series below 1e-3
__device__ __forceinline__ float coulomb_kernel(float4 p, float4 o, float mu) {
    const float dx = p.x - o.x, dy = p.y - o.y, dz = p.z - o.z;
    const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (r < ES_SMALL_R) {
        const float x = mu * r;
        return (mu * ES_TWO_OVER_SQRT_PI) * (1.f - (x * x) / 3.f);
    }
    return erff(mu * r) / r;
}

__global__ __launch_bounds__(ES_MAXP) void k_esp_overlap(
    const float* __restrict__ ref_xyz, const float* __restrict__ ref_q, int P, const float* __restrict__ xyz,
    const float* __restrict__ q, const int32_t* __restrict__ n_points, int PW, float mu, const float* __restrict__ e_rr,
    float* __restrict__ cross_out, float* __restrict__ self_out, float* __restrict__ tanimoto_out) {
    __shared__ float4 ref_s[ES_MAXP], own_s[ES_MAXP];
    __shared__ double cross_s[ES_MAXP], self_s[ES_MAXP];
    __shared__ int bad_s;

    const int b = blockIdx.x, t = threadIdx.x;
    const int np = min(max(n_points[b], 0), PW);
    if (t == 0) bad_s = 0;
    if (t < P) ref_s[t] = make_float4(ref_xyz[t * 3], ref_xyz[t * 3 + 1], ref_xyz[t * 3 + 2], ref_q[t]);
    float4 mine = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < np) {
        const float* p = xyz + ((size_t)b * PW + t) * 3;
        mine = make_float4(p[0], p[1], p[2], q[(size_t)b * PW + t]);
    }
    own_s[t] = mine;
    __syncthreads();
    if (t < np && !(isfinite(mine.x) && isfinite(mine.y) && isfinite(mine.z) && isfinite(mine.w))) bad_s = 1;

    double cross = 0.0, self = 0.0;
    if (t < np) {
        for (int j = 0; j < P; ++j) {
            const float4 o = ref_s[j];
            cross += (double)((mine.w * o.w) * coulomb_kernel(mine, o, mu));
        }
        for (int j = 0; j < np; ++j) {
            const float4 o = own_s[j];
            self += (double)((mine.w * o.w) * coulomb_kernel(mine, o, mu));
        }
    }
    cross_s[t] = cross;
    self_s[t] = self;
    __syncthreads();
    for (int s = ES_MAXP / 2; s > 0; s >>= 1) {       // the one tree: t takes t + s
        if (t < s) {
            cross_s[t] += cross_s[t + s];
            self_s[t] += self_s[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float nan = __int_as_float(0x7fc00000);
        const float c = (float)cross_s[0], m = (float)self_s[0];
        const float rr = e_rr != nullptr ? e_rr[0] : m;
        const float den = (rr + m) - c;
        const bool bad = bad_s != 0;
        cross_out[b] = bad ? nan : c;
        self_out[b] = bad ? nan : m;
        tanimoto_out[b] = bad ? nan : (den < ES_EMPTY ? 0.f : c / den);
    }
}

}  // namespace

extern "C" int mcg_charges_peoe(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, const uint8_t* types,
                                const uint64_t* ring_mask, const int32_t* n_rings, int B, int W, float* q_out,
                                float* qh_out, int32_t* nh_out, int32_t* status_out, void* stream) {
    if (!z || !bonds || !n_nodes_dev || !types || !ring_mask || !n_rings || !q_out || !qh_out || !nh_out || !status_out ||
        B < 0 || B > MCG_CHARGES_MAX_B || W < 1 || W > PE_MAXW) {
        mcg_set_error("mcg_charges_peoe: bad arguments (non-null z, bonds, n_nodes, types, ring_mask, n_rings, q_out, qh_out, "
                      "nh_out and status_out, 0 <= B <= %d, 1 <= W <= %d)", MCG_CHARGES_MAX_B, PE_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_charges_peoe, dim3((unsigned)((B + PE_MOLS - 1) / PE_MOLS)), dim3(PE_MAXW * PE_MOLS), 0,
                       (hipStream_t)stream, z, bonds, n_nodes_dev, types, reinterpret_cast<const u64*>(ring_mask), n_rings, B,
                       W, q_out, qh_out, nh_out, status_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_esp_overlap(const float* ref_xyz, const float* ref_q, int P, const float* xyz, const float* q,
                               const int32_t* n_points, int B, int PW, float mu, const float* e_rr, float* cross_out,
                               float* self_out, float* tanimoto_out, void* stream) {
    if (!ref_xyz || !ref_q || !xyz || !q || !n_points || !cross_out || !self_out || !tanimoto_out || B < 0 ||
        B > MCG_ESP_MAX_B || P < 1 || P > ES_MAXP || PW < 1 || PW > ES_MAXP || !(mu > 0.f) || !isfinite(mu)) {
        mcg_set_error("mcg_esp_overlap: bad arguments (non-null ref_xyz, ref_q, xyz, q, n_points, cross_out, self_out and "
                      "tanimoto_out, 0 <= B <= %d, 1 <= P <= %d, 1 <= PW <= %d, mu positive and finite)", MCG_ESP_MAX_B, ES_MAXP,
                      ES_MAXP);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_esp_overlap, dim3((unsigned)B), dim3(ES_MAXP), 0, (hipStream_t)stream, ref_xyz, ref_q, P, xyz, q,
                       n_points, PW, mu, e_rr, cross_out, self_out, tanimoto_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
