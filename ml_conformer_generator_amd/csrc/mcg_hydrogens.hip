// Explicit hydrogens ("Explicit hydrogens"): how many hydrogens each heavy atom of a molecular graph
// carries and where they sit.  The package's OWN definition - not RDKit's AddHs: no charges, no tautomer search.  The
// count is the pharmacophore perception's nH plus one aromatic N-H per 5-ring; the hybridisation is the force field's
// centre rule plus conjugation; the positions are ideal directions around the parent at rcov(Z) + 0.31 A.
//   k_hydrogens_place: one 64-lane workgroup (one wave) per molecule, lane = heavy atom, the layout of k_pharm_perceive:
//     stage   coordinates (float4) and bond codes (68-byte rows) -> LDS; the perceived ring masks -> LDS.
//     count   per lane deg, v2, the code counts, the hybridisation and nH; what a rule asks of OTHER atoms (a neighbour
//             with a code-2 or code-4 bond; the aromatic N of degree 2 that carry the donor bit) is one ballot each.  The
//             5-ring N-H rule is a walk over the ring list that every lane takes alike (at most 32 masks).
//     offsets an inclusive wave scan of the placed counts (shuffles, no atomics): atom a's hydrogens are the slots
//             off .. off + placed - 1, which IS the output order (ascending parent, then m).
//     fixed   every lane whose atom is not a rotor writes its hydrogens into the LDS slot list.
//     rotors  a rotor lane stores its frame (a, e1, e2), bond length and neighbour; the rotors are ranked by a ballot.
//             The scan then runs over (rotor, delta) PAIRS spread across the 64 lanes, pair = 12 * rank + delta / 30,
//             not over the rotor lanes alone: a drug-like molecule of 25 atoms has some 6-10 rotors, so the rotor lanes
//             alone would leave five lanes in six idle through the one loop of the kernel that does real arithmetic
//             (12 delta x <= 3 hydrogens x (n + fixed) distances each), while the pairs fill the wave (8 rotors: 96
//             pairs, two passes of one delta each).  Every pair's S is one lane's own sum in the one order of the
//             definition, so the spreading changes no bit.  S goes to LDS; the rotor's lane takes the smallest, ties to
//             the smallest delta, and writes its hydrogens.
//     write   plain stores: the slot list, the parents (-1 beyond the count), the per-atom counts and the row's totals.
//   Products and sums are rounded one by one (no contraction), square roots and divisions are correctly rounded, and every
//   loop bound is the molecule's own n or count: a molecule's result has the same bits whatever the batch, its row and the
//   padded widths.  No atomics, no inline assembly, no private arrays (no scratch).
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_elements.h"
#include "mcg_graph_rules.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int HY_MAXW = MCG_HYDROGENS_MAX_ATOMS;     // atoms per molecule: one lane and one mask bit each
constexpr int HY_SLOTS = 3 * HY_MAXW;                // hydrogens per molecule: 3 per atom that has a neighbour (4 if n == 1)
constexpr int HY_DELTAS = 12;                        // rotor candidates: 0, 30, ... 330 degrees
constexpr int HY_MAX_RINGS = MCG_PHARM_MAX_RINGS;
static_assert(HY_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");

enum : int { HY_TETRAHEDRAL = MCG_CLASS_TETRAHEDRAL, HY_PLANAR = MCG_CLASS_PLANAR, HY_LINEAR = MCG_CLASS_LINEAR };

constexpr float HY_XH = 0.31f;                       // X-H = rcov(Z) + 0.31 A
constexpr float HY_DEGENERATE = 1e-3f;
constexpr float HY_COS_HALF = 0.577350416216075f, HY_SIN_HALF = 0.8164964769643069f;      // 54.7356 deg
constexpr float HY_COS_TET = -0.33333299379025f, HY_SIN_TET = 0.942809161628603f;         // 109.4712 deg
constexpr float HY_COS_120 = -0.5f, HY_SIN_120 = 0.8660254037844387f;
constexpr float HY_HEAVY_REACH = 2.4f, HY_H_REACH = 2.0f;
constexpr float HY_INV_SQRT3 = 0.5773502691896258f;

__constant__ McgElementTable c_hyd_elements = MCG_ELEMENTS;
// cos, sin of 0, 30, ... 330 degrees
__constant__ float c_hyd_cos[HY_DELTAS] = {1.f, 0.8660254037844387f, 0.5f, 0.f, -0.5f, -0.8660254037844387f,
                                           -1.f, -0.8660254037844387f, -0.5f, 0.f, 0.5f, 0.8660254037844387f};
__constant__ float c_hyd_sin[HY_DELTAS] = {0.f, 0.5f, 0.8660254037844387f, 1.f, 0.8660254037844387f, 0.5f,
                                           0.f, -0.5f, -0.8660254037844387f, -1.f, -0.8660254037844387f, -0.5f};

struct V3 {
    float x, y, z;
};

__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 scale(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float norm(V3 a) { return sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// v / |v|; the zero vector stays zero
__device__ __forceinline__ V3 normalize(V3 a) {
    const float len = norm(a);
    return scale(len > 0.f ? 1.f / len : 0.f, a);
}
// normalize(e - (a.e) a), e the coordinate axis with the smallest |a.e| (ties: x, then y, then z)
__device__ __forceinline__ V3 perp(V3 a) {
    const float ax = fabsf(a.x), ay = fabsf(a.y), az = fabsf(a.z);
    int axis = 0;
    float least = ax;
    if (ay < least) axis = 1, least = ay;
    if (az < least) axis = 2;
    const V3 e = v3(axis == 0 ? 1.f : 0.f, axis == 1 ? 1.f : 0.f, axis == 2 ? 1.f : 0.f);
    return normalize(sub(e, scale(dot(a, e), a)));
}
__device__ __forceinline__ V3 xyz(float4 p) { return v3(p.x, p.y, p.z); }

// hydrogen m of a rotor at candidate d (delta = 30 d degrees): x + L (cos t a + sin t (cos phi e1 + sin phi e2)), t the
// H-X-j angle, phi = 180 + 120 m + delta (tetrahedral) or 180 + 180 m + delta (planar)
__device__ __forceinline__ V3 rotor_hydrogen(V3 x, V3 a, V3 e1, V3 e2, float len, bool planar, int m, int d) {
    const int t = (6 + (planar ? 6 : 4) * m + d) % HY_DELTAS;
    const V3 q = add(scale(c_hyd_cos[t], e1), scale(c_hyd_sin[t], e2));
    const V3 dir = add(scale(planar ? HY_COS_120 : HY_COS_TET, a), scale(planar ? HY_SIN_120 : HY_SIN_TET, q));
    return add(x, scale(len, dir));
}

__device__ __forceinline__ float shortfall2(V3 p, V3 q, float reach) {
    const float t = fmaxf(0.f, reach - norm(sub(p, q)));
    return t * t;
}

__global__ __launch_bounds__(HY_MAXW) void k_hydrogens_place(
    const float* __restrict__ coords, const int32_t* __restrict__ z, const int8_t* __restrict__ bonds,
    const int32_t* __restrict__ n_nodes, const uint8_t* __restrict__ types, const u64* __restrict__ ring_mask,
    const int32_t* __restrict__ n_rings, int N, int W, int HW, float* __restrict__ h_xyz_out,
    int32_t* __restrict__ h_parent_out, int32_t* __restrict__ h_count_out, int32_t* __restrict__ n_h_out,
    int32_t* __restrict__ unplaced_out, int32_t* __restrict__ rotor_delta_out) {
    __shared__ __attribute__((aligned(16))) uint8_t code[HY_MAXW * MCG_CODE_STRIDE];
    __shared__ float4 xs[HY_MAXW];                    // heavy atoms
    __shared__ float4 hx[HY_SLOTS];                   // hydrogens in output order; w = 1: fixed, 0: a rotor's
    __shared__ float4 fa[HY_MAXW], fe1[HY_MAXW], fe2[HY_MAXW];       // a rotor's frame, by atom; fa.w = its X-H length
    __shared__ u64 nbr[HY_MAXW];
    __shared__ u64 rings[HY_MAX_RINGS];
    __shared__ float score[HY_MAXW * HY_DELTAS];
    __shared__ int32_t parent[HY_SLOTS];
    __shared__ uint8_t rot_atom[HY_MAXW];             // the rotors in ascending atom index
    __shared__ uint8_t rot_info[HY_MAXW];             // by atom: hydrogens (1..3) | planar << 2
    __shared__ uint8_t rot_j[HY_MAXW];                // by atom: the rotor's one neighbour

    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), min(N, W));
    const bool real = a < n;

    // the molecule's W x W codes -> LDS rows; the diagonal, the padding and every code outside 1..4 become 0
    mcg_stage_codes(code, bonds + (size_t)b * W * W, W, n, a, HY_MAXW);
    float4 xa = make_float4(0.f, 0.f, 0.f, 0.f);
    if (real) {
        const float* p = coords + ((size_t)b * N + a) * 3;
        xa = make_float4(p[0], p[1], p[2], 0.f);
    }
    xs[a] = xa;
    const bool bad = __ballot(real && !(isfinite(xa.x) && isfinite(xa.y) && isfinite(xa.z))) != 0ull;
    const u64 live = low_bits(n);
    const int nr = min(max(n_rings[b], 0), HY_MAX_RINGS);
    if (a < HY_MAX_RINGS) rings[a] = a < nr ? (ring_mask[(size_t)b * HY_MAX_RINGS + a] & live) : 0ull;
    for (int s = a; s < HY_SLOTS; s += HY_MAXW) {
        hx[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        parent[s] = -1;
    }
    __syncthreads();

    const int za = real ? z[(size_t)b * W + a] : 0;
    const int ta = real ? types[(size_t)b * W + a] : 0;
    // the count and class rules (mcg_graph_rules.h, shared with k_charges_peoe)
    const McgBondTally tally = mcg_bond_tally(code + a * MCG_CODE_STRIDE, real ? n : 0);
    const u64 mine = tally.mask;
    const int deg = tally.deg;
    nbr[a] = mine;
    const u64 m_has24 = __ballot(real && mcg_has_code_2_or_4(tally));
    const u64 m_ring_n = __ballot(real && mcg_ring_nh_candidate(za, tally, ta));
    const int hyb = mcg_parent_class(za, tally, m_has24);
    int nh = mcg_implicit_hydrogens(real, a, za, tally, rings, nr, m_ring_n);

    // how many of them this definition places
    const int k = deg;
    int placed = 0;
    if (hyb == HY_TETRAHEDRAL)
        placed = (k == 3 && nh == 1) || (k == 2 && nh <= 2) || (k == 1 && nh <= 3) || (k == 0 && n == 1 && nh <= 4) ? nh : 0;
    else if (hyb == HY_PLANAR)
        placed = (k == 2 && nh == 1) || (k == 1 && nh <= 2) || (k == 0 && n == 1 && nh <= 3) ? nh : 0;
    else
        placed = (k == 1 && nh == 1) || (k == 0 && n == 1 && nh <= 2) ? nh : 0;
    if (bad) placed = 0, nh = 0;
    const bool rotor = k == 1 && hyb != HY_LINEAR && placed >= 1;

    int incl = placed;
    for (int off = 1; off < HY_MAXW; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (a >= off) incl += v;
    }
    const int total = __shfl(incl, HY_MAXW - 1);
    const int first = incl - placed;
    const int missing = wave_sum(nh - placed);

    float rc = 0.f;
    if (real && za >= 0 && za < MCG_N_ELEMENT_Z) rc = (float)c_hyd_elements.rcov[za];
    const float len = rc + HY_XH;
    const V3 x = xyz(xa);
    __syncthreads();                                  // nbr

    auto put = [&](int m, V3 dir, float fixed) {
        const V3 p = add(x, scale(len, dir));
        hx[first + m] = make_float4(p.x, p.y, p.z, fixed);
    };
    auto unit_to = [&](int j) { return normalize(sub(xyz(xs[j]), x)); };
    for (int m = 0; m < placed; ++m) parent[first + m] = a;

    if (placed >= 1 && !rotor) {
        if (k == 0) {
            if (hyb == HY_TETRAHEDRAL) {
                const float s = HY_INV_SQRT3;
                put(0, v3(s, s, s), 1.f);
                if (placed >= 2) put(1, v3(s, -s, -s), 1.f);
                if (placed >= 3) put(2, v3(-s, s, -s), 1.f);
                if (placed >= 4) put(3, v3(-s, -s, s), 1.f);
            } else if (hyb == HY_PLANAR) {
                put(0, v3(1.f, 0.f, 0.f), 1.f);
                if (placed >= 2) put(1, v3(HY_COS_120, HY_SIN_120, 0.f), 1.f);
                if (placed >= 3) put(2, v3(HY_COS_120, -HY_SIN_120, 0.f), 1.f);
            } else {
                put(0, v3(1.f, 0.f, 0.f), 1.f);
                if (placed >= 2) put(1, v3(-1.f, 0.f, 0.f), 1.f);
            }
        } else if (k == 1) {                          // linear
            put(0, neg(unit_to(low_bit(mine))), 1.f);
        } else {
            const int j1 = low_bit(mine);
            const u64 rest = mine & (mine - 1ull);
            const int j2 = low_bit(rest);
            const V3 u1 = unit_to(j1), u2 = unit_to(j2);
            if (k == 3) {
                const V3 u3 = unit_to(low_bit(rest & (rest - 1ull)));
                const V3 s = add(add(u1, u2), u3);
                put(0, norm(s) < HY_DEGENERATE ? normalize(cross(sub(u2, u1), sub(u3, u1))) : neg(normalize(s)), 1.f);
            } else {
                const V3 s = add(u1, u2);
                if (hyb == HY_PLANAR) {
                    put(0, norm(s) < HY_DEGENERATE ? perp(u1) : neg(normalize(s)), 1.f);
                } else {
                    const V3 c = cross(u1, u2);
                    V3 bis, nrm;
                    if (norm(s) < HY_DEGENERATE || norm(c) < HY_DEGENERATE) {
                        bis = perp(u1);
                        nrm = cross(u1, bis);
                    } else {
                        bis = neg(normalize(s));
                        nrm = normalize(c);
                    }
                    put(0, add(scale(HY_COS_HALF, bis), scale(HY_SIN_HALF, nrm)), 1.f);
                    if (placed >= 2) put(1, sub(scale(HY_COS_HALF, bis), scale(HY_SIN_HALF, nrm)), 1.f);
                }
            }
        }
    }
    if (rotor) {                                      // its frame; the slots keep w = 0 until the scan has chosen
        const int j = low_bit(mine);
        const V3 xj = xyz(xs[j]);
        const V3 av = normalize(sub(xj, x));
        const u64 others = nbr[j] & ~(1ull << a);
        V3 p = v3(0.f, 0.f, 0.f);
        if (others != 0ull) {
            const V3 d = sub(xyz(xs[low_bit(others)]), xj);
            p = sub(d, scale(dot(d, av), av));
        }
        if (others == 0ull || norm(p) < HY_DEGENERATE) p = perp(av);
        const V3 e1 = normalize(p), e2 = cross(av, e1);
        fa[a] = make_float4(av.x, av.y, av.z, len);
        fe1[a] = make_float4(e1.x, e1.y, e1.z, 0.f);
        fe2[a] = make_float4(e2.x, e2.y, e2.z, 0.f);
        rot_info[a] = (uint8_t)(placed | (hyb == HY_PLANAR ? 4 : 0));
        rot_j[a] = (uint8_t)j;
    }
    const u64 m_rotor = __ballot(rotor);
    const int n_rotors = __popcll(m_rotor);
    if (rotor) rot_atom[__popcll(m_rotor & low_bits(a))] = (uint8_t)a;
    __syncthreads();

    // S(delta) of every (rotor, delta) pair, one pair per lane and pass
    for (int pair = a; pair < n_rotors * HY_DELTAS; pair += HY_MAXW) {
        const int r = pair / HY_DELTAS, d = pair - r * HY_DELTAS;
        const int atom = rot_atom[r], info = rot_info[atom], j = rot_j[atom];
        const bool planar = (info & 4) != 0;
        if (planar && d != 0 && d != 6) continue;     // a planar rotor has two candidates: 0 and 180 degrees
        const int h = info & 3;
        const float4 f = fa[atom];
        const V3 px = xyz(xs[atom]), av = xyz(f), e1 = xyz(fe1[atom]), e2 = xyz(fe2[atom]);
        float S = 0.f;
        for (int m = 0; m < h; ++m) {
            const V3 p = rotor_hydrogen(px, av, e1, e2, f.w, planar, m, d);
            for (int i = 0; i < n; ++i)
                if (i != atom && i != j) S = S + shortfall2(p, xyz(xs[i]), HY_HEAVY_REACH);
            for (int s = 0; s < total; ++s) {
                const float4 q = hx[s];
                if (q.w != 0.f) S = S + shortfall2(p, xyz(q), HY_H_REACH);
            }
        }
        score[pair] = S;
    }
    __syncthreads();

    int delta = -1;
    if (rotor) {
        const float* mine_s = score + __popcll(m_rotor & low_bits(a)) * HY_DELTAS;
        const bool planar = hyb == HY_PLANAR;
        int best = 0;
        float least = mine_s[0];
        for (int d = planar ? 6 : 1; d < HY_DELTAS; d += planar ? 6 : 1)
            if (mine_s[d] < least) best = d, least = mine_s[d];
        delta = 30 * best;
        const V3 av = xyz(fa[a]), e1 = xyz(fe1[a]), e2 = xyz(fe2[a]);
        for (int m = 0; m < placed; ++m) {
            const V3 p = rotor_hydrogen(x, av, e1, e2, len, planar, m, best);
            hx[first + m] = make_float4(p.x, p.y, p.z, 0.f);
        }
    }
    __syncthreads();

    float* out = h_xyz_out + (size_t)b * HW * 3;
    int32_t* pout = h_parent_out + (size_t)b * HW;
    for (int s = a; s < HW; s += HY_MAXW) {
        const bool w = s < total;                     // total <= max(4, 3 n) <= HW
        const float4 p = w ? hx[s] : make_float4(0.f, 0.f, 0.f, 0.f);
        out[s * 3] = p.x;
        out[s * 3 + 1] = p.y;
        out[s * 3 + 2] = p.z;
        pout[s] = w ? parent[s] : -1;
    }
    if (a < W) {
        h_count_out[(size_t)b * W + a] = placed;
        if (rotor_delta_out != nullptr) rotor_delta_out[(size_t)b * W + a] = delta;
    }
    if (a == 0) {
        n_h_out[b] = bad ? -1 : total;
        unplaced_out[b] = missing;
    }
}

}  // namespace

extern "C" int mcg_hydrogens_place(const float* coords, const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                                   const uint8_t* types, const uint64_t* ring_mask, const int32_t* n_rings, int B, int N,
                                   int W, int HW, float* h_xyz_out, int32_t* h_parent_out, int32_t* h_count_out,
                                   int32_t* n_h_out, int32_t* unplaced_out, int32_t* rotor_delta_out, void* stream) {
    if (!coords || !z || !bonds || !n_nodes_dev || !types || !ring_mask || !n_rings || !h_xyz_out || !h_parent_out ||
        !h_count_out || !n_h_out || !unplaced_out || B < 0 || B > MCG_HYDROGENS_MAX_B || N < 1 || W < 1 || W > HY_MAXW ||
        HW < 4 || HW < 3 * W) {
        mcg_set_error("mcg_hydrogens_place: bad arguments (non-null coords, z, bonds, n_nodes, types, ring_mask, n_rings, "
                      "h_xyz_out, h_parent_out, h_count_out, n_h_out and unplaced_out, 0 <= B <= %d, N >= 1, 1 <= W <= %d, "
                      "HW >= max(4, 3 W))", MCG_HYDROGENS_MAX_B, HY_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_hydrogens_place, dim3((unsigned)B), dim3(HY_MAXW), 0, (hipStream_t)stream, coords, z, bonds,
                       n_nodes_dev, types, reinterpret_cast<const u64*>(ring_mask), n_rings, N, W, HW, h_xyz_out,
                       h_parent_out, h_count_out, n_h_out, unplaced_out, rotor_delta_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
