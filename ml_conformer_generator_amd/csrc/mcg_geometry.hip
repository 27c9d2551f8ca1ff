// Relaxed geometry ("Relaxed geometry"): the heavy atoms of every molecule are moved downhill on a
// small restrained valence force field.  The package's OWN force field - a labelled substitute, NOT MMFF94: harmonic
// distance terms only (bonds, 1-3 "angle" distances, a one-sided non-bonded floor) plus the reference's flat-bottomed
// position restraint (0.2 A, 800 kcal/mol/A^2); no torsions, no impropers, no charges, no hydrogens.
//   k_geometry_relax: one 64-lane workgroup (one wave) per molecule, lane = atom.
//     setup   the bond codes -> LDS rows (68-byte stride), the 64-bit neighbour masks and each atom's cos(theta0); then
//             lane i fills row i of the pair tables: class (none / bond / angle / non-bonded, one byte) and d0 (fp32, rows
//             of 65 floats, so the lanes of a wave walking column j of their own rows hit different banks).
//     eval    lane i sums its atom's energy share and gradient over j = 0 .. n-1 in that order (x_j is one broadcast
//             16-byte LDS read); every pair is seen from both ends, so each end takes half the pair energy.  No atomics.
//     reduce  the energy (sum) and the largest atom gradient (max) go through a fixed xor butterfly over the 64 lanes:
//             fp32 addition and maximum are commutative, so every lane ends with the same bits, holds the same E and step
//             length and takes the same accept / reject branch.
//     step    x' = x - (s / max_i |g_i|) g from s = 0.02 A; E(x') < E(x): accept, s *= 1.2; else keep x, s *= 0.5.  The
//             trial coordinates go to the other of two LDS buffers; accepting swaps the buffers.
//   Products and sums are rounded one by one (no contraction).  A molecule's outputs depend on its own atoms only: the
//   lane count, the loop bounds (n) and every order of summation are fixed, whatever the batch, row or padded widths.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_elements.h"
#include "mcg_graph_rules.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int GR_MAXW = MCG_RELAX_MAX_ATOMS;     // atoms per molecule: one lane and one 64-bit neighbour mask each
constexpr int GR_DSTRIDE = 65;                   // floats per row of the d0 table
static_assert(GR_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");

// the force field (tests/geometry_ref.py restates it in fp64)
constexpr float GR_K_BOND = 600.f, GR_K_ANGLE = 150.f, GR_K_NONBONDED = 100.f;
constexpr float GR_SHRINK_AROMATIC = 0.13f, GR_SHRINK_DOUBLE = 0.18f, GR_SHRINK_TRIPLE = 0.32f;
constexpr float GR_NONBONDED_MARGIN = 0.9f;
constexpr float GR_RESTRAINT_FLAT = 0.2f, GR_RESTRAINT_K = 800.f;
constexpr float GR_COS_180 = -1.f, GR_COS_120 = -0.5f, GR_COS_TETRAHEDRAL = -0.33331324756823727f /* 109.47 deg */,
                GR_COS_108 = -0.30901699437494734f, GR_COS_90 = 0.f;
constexpr float GR_STEP0 = 0.02f, GR_GROW = 1.2f, GR_SHRINK = 0.5f;

enum : uint8_t { GR_NONE = 0, GR_BOND = 1, GR_ANGLE = 2, GR_NONBONDED = 3 };

__constant__ McgElementTable c_relax_elements = MCG_ELEMENTS;

struct RelaxShared {
    uint8_t code[GR_MAXW * MCG_CODE_STRIDE];     // bond codes 0 / 1 / 2 / 3 / 4, zero on the diagonal and the padding
    uint8_t cls[GR_MAXW * MCG_CODE_STRIDE];      // pair classes
    float d0[GR_MAXW * GR_DSTRIDE];
    unsigned long long nbr[GR_MAXW];
    float rcov[GR_MAXW];
    float cos0[GR_MAXW];                         // cos(theta0) of the atom as an angle centre
    float4 x[2][GR_MAXW];                        // the accepted and the trial coordinates
};

__device__ __forceinline__ float bond_d0(const RelaxShared& sh, int i, int j) {
    const uint32_t c = sh.code[i * MCG_CODE_STRIDE + j];
    const float shrink = c == 4 ? GR_SHRINK_AROMATIC : c == 2 ? GR_SHRINK_DOUBLE : c == 3 ? GR_SHRINK_TRIPLE : 0.f;
    return (sh.rcov[i] + sh.rcov[j]) - shrink;
}

struct AtomEval {
    float e, gx, gy, gz;          // this atom's share of E (half of each of its pair terms, its restraint) and dE/dx_i
};

// Energy share and gradient of atom i at the coordinates x (lane i's own: xi), restrained to x0i.
__device__ __forceinline__ AtomEval eval_atom(const RelaxShared& sh, const float4* __restrict__ x, int i, int n, bool real,
                                              float4 xi, float4 x0i) {
    AtomEval r = {0.f, 0.f, 0.f, 0.f};
    if (!real) return r;
    const float* d0row = sh.d0 + i * GR_DSTRIDE;
    const uint8_t* crow = sh.cls + i * MCG_CODE_STRIDE;
#pragma unroll 4                 // four independent sqrt / divide chains in flight; the sums keep their order
    for (int j = 0; j < n; ++j) {
        const float4 xj = x[j];
        const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
        const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float diff = dist - d0row[j];
        const uint32_t c = crow[j];
        const float k = c == GR_BOND ? GR_K_BOND : c == GR_ANGLE ? GR_K_ANGLE
                        : (c == GR_NONBONDED && diff < 0.f) ? GR_K_NONBONDED : 0.f;
        const float kd = k * diff;
        r.e = r.e + (0.25f * kd) * diff;
        const float f = dist > 0.f ? kd / dist : 0.f;
        r.gx = r.gx + f * dx;
        r.gy = r.gy + f * dy;
        r.gz = r.gz + f * dz;
    }
    const float ux = xi.x - x0i.x, uy = xi.y - x0i.y, uz = xi.z - x0i.z;
    const float u = sqrtf((ux * ux + uy * uy) + uz * uz);
    const float over = fmaxf(u - GR_RESTRAINT_FLAT, 0.f);
    const float ko = GR_RESTRAINT_K * over;
    r.e = r.e + (0.5f * ko) * over;
    const float f = u > 0.f ? ko / u : 0.f;
    r.gx = r.gx + f * ux;
    r.gy = r.gy + f * uy;
    r.gz = r.gz + f * uz;
    return r;
}

__global__ __launch_bounds__(GR_MAXW) void k_geometry_relax(const float* __restrict__ coords,
                                                            const float* __restrict__ restraint_ref,
                                                            const int32_t* __restrict__ z,
                                                            const int8_t* __restrict__ bonds,
                                                            const int32_t* __restrict__ n_nodes, int N, int W, int steps,
                                                            float* __restrict__ coords_out, float* __restrict__ energy_out,
                                                            float* __restrict__ grad_out, float* __restrict__ stats_out) {
    __shared__ RelaxShared sh;
    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), min(W, N));
    const bool real = a < n;

    mcg_stage_codes(sh.code, bonds + (size_t)b * W * W, W, n, a, GR_MAXW);
    float rc = 0.f;
    if (real) {
        const int zi = z[(size_t)b * W + a];
        rc = zi >= 0 && zi < MCG_N_ELEMENT_Z ? (float)c_relax_elements.rcov[zi] : 0.f;
    }
    sh.rcov[a] = rc;
    const bool unknown = __any(real && !(rc > 0.f)) != 0;          // an element without a radius: the row is not relaxed
    __syncthreads();

    {   // neighbour mask and cos(theta0) of atom a as an angle centre
        const McgBondTally t = mcg_bond_tally(sh.code + a * MCG_CODE_STRIDE, real ? n : 0);
        sh.nbr[a] = t.mask;
        sh.cos0[a] = (t.n3 >= 1 || t.n2 >= 2) ? GR_COS_180 : (t.n2 == 1 || t.narom >= 1) ? GR_COS_120 : GR_COS_TETRAHEDRAL;
    }
    __syncthreads();

    if (real) {   // row a of the pair tables
        const unsigned long long mine = sh.nbr[a];
        for (int k = 0; k < n; ++k) {
            uint8_t cl = GR_NONE;
            float d = 0.f;
            const unsigned long long common = mine & sh.nbr[k];
            if (k == a) {
            } else if (sh.code[a * MCG_CODE_STRIDE + k] != 0) {
                cl = GR_BOND;
                d = bond_d0(sh, a, k);
            } else if (common != 0ull) {
                cl = GR_ANGLE;
                d = INFINITY;
                const bool four_ring = __popcll(common) >= 2;
                for (unsigned long long todo = common; todo != 0ull; todo &= todo - 1ull) {
                    const int j = low_bit(todo);
                    float c = sh.cos0[j];
                    if (four_ring) {
                        c = GR_COS_90;
                    } else {                 // a path a - p - q - k that avoids j closes a five-ring through j
                        const unsigned long long jbit = 1ull << j, far = sh.nbr[k] & ~jbit;
                        bool five_ring = false;
                        for (unsigned long long p = mine & ~jbit; p != 0ull; p &= p - 1ull)
                            five_ring = five_ring || (sh.nbr[low_bit(p)] & far) != 0ull;
                        if (five_ring) c = fmaxf(c, GR_COS_108);
                    }
                    const float la = bond_d0(sh, a, j), lb = bond_d0(sh, j, k);
                    d = fminf(d, sqrtf((la * la + lb * lb) - ((2.f * la) * lb) * c));
                }
            } else {
                cl = GR_NONBONDED;
                d = (sh.rcov[a] + sh.rcov[k]) + GR_NONBONDED_MARGIN;
            }
            sh.cls[a * MCG_CODE_STRIDE + k] = cl;
            sh.d0[a * GR_DSTRIDE + k] = d;
        }
    }

    float4 xi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (real) {
        const float* p = coords + ((size_t)b * N + a) * 3;
        xi = make_float4(p[0], p[1], p[2], 0.f);
    }
    float4 x0i = xi;
    if (real && restraint_ref != nullptr) {
        const float* p = restraint_ref + ((size_t)b * N + a) * 3;
        x0i = make_float4(p[0], p[1], p[2], 0.f);
    }
    const float4 xin = xi;
    int cur = 0;
    sh.x[0][a] = xi;
    __syncthreads();

    AtomEval ev = eval_atom(sh, sh.x[0], a, n, real, xi, x0i);
    float E = wave_sum(ev.e);
    float gmax = wave_max(sqrtf((ev.gx * ev.gx + ev.gy * ev.gy) + ev.gz * ev.gz));
    const float e_start = E;
    if (grad_out != nullptr) {
        float* g = grad_out + (size_t)b * N * 3;
        for (int p = a; p < N; p += GR_MAXW) {
            const bool w = p == a && real && !unknown;
            g[p * 3] = w ? ev.gx : 0.f;
            g[p * 3 + 1] = w ? ev.gy : 0.f;
            g[p * 3 + 2] = w ? ev.gz : 0.f;
        }
    }

    float s = GR_STEP0;
    int accepted = 0;
    if (!unknown) {
        for (int it = 0; it < steps; ++it) {
            if (!(gmax > 0.f)) break;                // a stationary point (or a non-finite gradient: nothing can be accepted)
            const float scale = s / gmax;
            const float4 xt = make_float4(xi.x - scale * ev.gx, xi.y - scale * ev.gy, xi.z - scale * ev.gz, 0.f);
            sh.x[cur ^ 1][a] = xt;
            __syncthreads();
            const AtomEval et = eval_atom(sh, sh.x[cur ^ 1], a, n, real, xt, x0i);
            const float Et = wave_sum(et.e);
            if (Et < E) {                            // the same bits in every lane: one branch for the wave
                xi = xt;
                ev = et;
                E = Et;
                gmax = wave_max(sqrtf((et.gx * et.gx + et.gy * et.gy) + et.gz * et.gz));
                cur ^= 1;
                ++accepted;
                s = s * GR_GROW;
            } else {
                s = s * GR_SHRINK;
            }
            __syncthreads();
        }
    }

    float* out = coords_out + (size_t)b * N * 3;
    for (int p = a; p < N; p += GR_MAXW) {
        const bool w = p == a && real;
        out[p * 3] = w ? xi.x : 0.f;
        out[p * 3 + 1] = w ? xi.y : 0.f;
        out[p * 3 + 2] = w ? xi.z : 0.f;
    }
    const float mx = xi.x - xin.x, my = xi.y - xin.y, mz = xi.z - xin.z;
    const float moved = wave_max(sqrtf((mx * mx + my * my) + mz * mz));
    if (a == 0) {
        const float nan = __builtin_nanf("");
        energy_out[(size_t)b * 2] = unknown ? nan : e_start;
        energy_out[(size_t)b * 2 + 1] = unknown ? nan : E;
        if (stats_out != nullptr) {
            stats_out[(size_t)b * 2] = (float)accepted;
            stats_out[(size_t)b * 2 + 1] = moved;
        }
    }
}

}  // namespace

extern "C" int mcg_geometry_relax_ex(const float* coords, const float* restraint_ref, const int32_t* z, const int8_t* bonds,
                                     const int32_t* n_nodes_dev, int B, int N, int W, int steps, float* coords_out,
                                     float* energy_out, float* grad_out, float* stats_out, void* stream) {
    if (!coords || !z || !bonds || !n_nodes_dev || !coords_out || !energy_out || B < 0 || N < 1 || W < 1 ||
        W > MCG_RELAX_MAX_ATOMS || steps < 0 || steps > MCG_RELAX_MAX_STEPS) {
        mcg_set_error("mcg_geometry_relax: bad arguments (non-null coords, z, bonds, n_nodes, coords_out and energy_out, "
                      "B >= 0, N >= 1, 1 <= W <= %d, 0 <= steps <= %d)", MCG_RELAX_MAX_ATOMS, MCG_RELAX_MAX_STEPS);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_geometry_relax, dim3((unsigned)B), dim3(GR_MAXW), 0, (hipStream_t)stream, coords, restraint_ref, z,
                       bonds, n_nodes_dev, N, W, steps, coords_out, energy_out, grad_out, stats_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_geometry_relax(const float* coords, const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                                  int B, int N, int W, int steps, float* coords_out, float* energy_out, float* grad_out,
                                  float* stats_out, void* stream) {
    return mcg_geometry_relax_ex(coords, nullptr, z, bonds, n_nodes_dev, B, N, W, steps, coords_out, energy_out, grad_out,
                                 stats_out, stream);
}
