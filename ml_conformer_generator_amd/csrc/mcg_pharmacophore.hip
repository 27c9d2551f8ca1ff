// Pharmacophore features of molecular graphs and their Gaussian overlap with a reference's features (DESIGN.md section
// 6, "Pharmacophore overlap").  The package's OWN definition - not RDKit's feature factory, not a vendor's colour force
// field.  Features: donor, acceptor, cation, anion, hydrophobe (per-atom bits 1 2 4 8 16) and one ring feature per
// aromatic ring; perceived from the heavy-atom graph alone (elements, bond codes 1 / 2 / 3 / 4 aromatic), never from
// coordinates, so perception is exact integer work.
//   k_pharm_perceive: one 64-lane workgroup (one wave) per molecule, lane = atom, the layout of k_graph_fingerprint: bond
//                     codes in LDS rows of 68 bytes, 64-bit neighbour masks.  What a rule asks of an atom's neighbours
//                     ("is aromatic", "is an O of degree 1", ...) is one wave ballot per property and an AND with the
//                     lane's own masks.  Rings: lane s walks the simple paths of ring-eligible atoms above s along
//                     aromatic bonds, five nested loops over masks (at most 3 * 2^4 = 48 paths, no per-lane array); a
//                     closed path of 5 or 6 counts once per direction (second atom < last atom) and once per member set
//                     (a set with chords has several closed paths: the lexicographically first, found by the same
//                     walk restricted to the set).  The masks go into an LDS list in arrival order and are then ranked
//                     by counting, which gives the ascending order whatever the arrival order was.
//   k_pharm_score:    one 64-lane workgroup per candidate.  The candidate's feature list (atoms in ascending index, bits
//                     in ascending order, then the rings at their fp32 centroids) and the reference's are staged in LDS.
//                     Lane l owns the candidate features l, l + 64, ...: per feature j the fp64 sum over the reference
//                     features of its type in ascending order of fp32 expf(-0.5 d2), d2 = dx*dx + dy*dy + dz*dz without
//                     contraction; the same against the candidate's own list.  Lane t < 6 then adds the per-feature
//                     sums of type t in ascending j, lane 0 the six types: one order, fixed by the two lists alone.
//                     coords == NULL: the candidate list IS the reference list - the run that yields O(R,R).
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_graph_rules.h"

namespace {

typedef unsigned long long u64;

constexpr int PH_MAXW = 64;                  // atoms per molecule: one lane and one mask bit each
constexpr int PH_MAX_RINGS = MCG_PHARM_MAX_RINGS;
constexpr int PH_MAX_FEAT = MCG_PHARM_MAX_FEATURES;
constexpr int PH_RING_CAP = PH_MAXW * 36;    // closed paths one lane can find: 24 / 2 of five atoms + 48 / 2 of six
constexpr int PH_T_RING = 5;                 // type index of a ring feature (atom bits: indices 0..4)
static_assert(PH_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");

// The closed paths of 5 or 6 atoms through s inside `allowed` (which does not hold s), in ascending nested order.
// found(member mask, path key) -> true stops the walk.  arom[x]: x's ring-eligible aromatic neighbours (<= 3 bits).
template <class F>
__device__ __forceinline__ void walk_rings(const u64* arom, int s, u64 allowed, F&& found) {
    const u64 sb = 1ull << s;
    for (u64 m1 = arom[s] & allowed; m1 != 0ull; m1 &= m1 - 1ull) {
        const int p1 = low_bit(m1);
        const u64 u1 = 1ull << p1;
        for (u64 m2 = arom[p1] & allowed & ~u1; m2 != 0ull; m2 &= m2 - 1ull) {
            const int p2 = low_bit(m2);
            const u64 u2 = u1 | (1ull << p2);
            for (u64 m3 = arom[p2] & allowed & ~u2; m3 != 0ull; m3 &= m3 - 1ull) {
                const int p3 = low_bit(m3);
                const u64 u3 = u2 | (1ull << p3);
                for (u64 m4 = arom[p3] & allowed & ~u3; m4 != 0ull; m4 &= m4 - 1ull) {
                    const int p4 = low_bit(m4);
                    const u64 u4 = u3 | (1ull << p4);
                    const u64 a4 = arom[p4];
                    const uint32_t k4 = (uint32_t)p1 | ((uint32_t)p2 << 6) | ((uint32_t)p3 << 12) | ((uint32_t)p4 << 18);
                    if ((a4 & sb) != 0ull && p1 < p4 && found(u4 | sb, k4 | (63u << 24))) return;
                    for (u64 m5 = a4 & allowed & ~u4; m5 != 0ull; m5 &= m5 - 1ull) {
                        const int p5 = low_bit(m5);
                        if ((arom[p5] & sb) != 0ull && p1 < p5 &&
                            found(u4 | (1ull << p5) | sb, k4 | ((uint32_t)p5 << 24)))
                            return;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(PH_MAXW) void k_pharm_perceive(const int32_t* __restrict__ z,
                                                            const int8_t* __restrict__ bonds,
                                                            const int32_t* __restrict__ n_nodes, int W,
                                                            uint8_t* __restrict__ types_out,
                                                            int32_t* __restrict__ n_rings_out,
                                                            u64* __restrict__ ring_out) {
    __shared__ __attribute__((aligned(16))) uint8_t code[PH_MAXW * MCG_CODE_STRIDE];
    __shared__ u64 arom[PH_MAXW];
    __shared__ u64 ring_list[PH_RING_CAP];
    __shared__ u64 sorted[PH_MAX_RINGS];
    __shared__ int ring_count;

    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), W);
    const bool real = a < n;

    mcg_stage_codes(code, bonds + (size_t)b * W * W, W, n, a, PH_MAXW);
    if (a == 0) ring_count = 0;
    if (a < PH_MAX_RINGS) sorted[a] = 0ull;
    __syncthreads();

    const int za = real ? z[(size_t)b * W + a] : 0;
    // its own row walk, not mcg_bond_tally: with the tally this kernel needs 83 VGPRs, not 79 - past the 80-register step
    const uint8_t* row = code + a * MCG_CODE_STRIDE;
    u64 mine = 0ull, single = 0ull, dbl = 0ull, multiple = 0ull, ar = 0ull;
    int deg = 0, v2 = 0, narom = 0;
    if (real) {
        for (int j = 0; j < n; ++j) {
            const int c = row[j];
            if (c != 0) {
                const u64 bit = 1ull << j;
                mine |= bit;
                ++deg;
                v2 += c == 1 ? 2 : c == 2 ? 4 : c == 3 ? 6 : 3;
                single |= c == 1 ? bit : 0ull;
                dbl |= c == 2 ? bit : 0ull;
                multiple |= (c == 2 || c == 3) ? bit : 0ull;
                if (c == 4) {
                    ar |= bit;
                    ++narom;
                }
            }
        }
    }
    const bool aromatic = narom >= 1;
    const bool eligible = real && narom >= 2 && narom <= 3 && deg <= 4;
    // one ballot per property a rule asks of OTHER atoms
    const u64 m_eligible = __ballot(eligible);
    const u64 m_aromatic = __ballot(aromatic);
    const u64 m_o_s = __ballot(za == 8 || za == 16);
    const u64 m_o_deg1 = __ballot(za == 8 && deg == 1);
    const u64 m_carbon = __ballot(za == 6);
    const u64 m_chalcogen = __ballot(za == 8 || za == 16 || za == 34);
    const u64 m_arom_n3 = __ballot(za == 7 && aromatic && deg == 3);
    const bool arom_n2 = za == 7 && aromatic && deg == 2;
    const u64 m_arom_n2 = __ballot(arom_n2);
    const u64 m_dbl_o_s = __ballot((dbl & m_o_s) != 0ull);        // atoms with a double bond to O or S

    arom[a] = eligible ? (ar & m_eligible) : 0ull;
    __syncthreads();

    // rings whose lowest member is this lane's atom
    if (eligible) {
        const u64 above = ~low_bits(a + 1);
        walk_rings(arom, a, above, [&](u64 mask, uint32_t key) {
            uint32_t first = ~0u;
            walk_rings(arom, a, mask & ~(1ull << a), [&](u64 m2, uint32_t k2) {
                if (m2 != mask) return false;
                first = k2;
                return true;
            });
            if (first == key) {
                const int slot = atomicAdd(&ring_count, 1);
                if (slot < PH_RING_CAP) ring_list[slot] = mask;
            }
            return false;
        });
    }
    __syncthreads();
    const int total = ring_count;
    const int listed = min(total, PH_RING_CAP);

    // ascending order by counting: the masks are distinct, so the ranks are too
    for (int e = a; e < listed; e += PH_MAXW) {
        const u64 m = ring_list[e];
        int rank = 0;
        for (int k = 0; k < listed; ++k) rank += ring_list[k] < m ? 1 : 0;
        if (rank < PH_MAX_RINGS) sorted[rank] = m;
    }

    int t = 0;
    const int nh = max(0, (2 * (za == 7 ? 3 : za == 8 ? 2 : 0) - v2) / 2);        // read for N and O only
    if ((za == 7 || za == 8) && !aromatic && nh >= 1) t |= 1;
    if (arom_n2) {
        bool donor = false, shared = false;
        for (int k = 0; k < listed; ++k) {
            const u64 m = ring_list[k];
            if ((m >> a & 1ull) != 0ull && __popcll(m) == 5 && (m & (m_chalcogen | m_arom_n3)) == 0ull) {
                donor = true;
                shared = shared || __popcll(m & m_arom_n2) >= 2;
            }
        }
        if (donor) t |= 1;
        if (!donor || shared) t |= 2;
    }
    if (za == 8 && narom == 0 && v2 <= 4) t |= 2;
    if (za == 7 && !aromatic && multiple != 0ull && v2 <= 6) t |= 2;
    if (za == 7 && !aromatic && deg >= 1 && single == mine && (mine & (m_aromatic | m_dbl_o_s)) == 0ull) t |= 4;
    if ((za == 6 || za == 16 || za == 15) && (dbl & m_o_deg1) != 0ull && (single & m_o_deg1) != 0ull) t |= 8;
    if (za == 6 && !aromatic && (mine & ~m_carbon) == 0ull) t |= 16;
    if (za == 17 || za == 35 || za == 53) t |= 16;
    if (a < W) types_out[(size_t)b * W + a] = real ? (uint8_t)t : (uint8_t)0;
    __syncthreads();
    if (a < PH_MAX_RINGS) ring_out[(size_t)b * PH_MAX_RINGS + a] = sorted[a];
    if (a == 0) n_rings_out[b] = total;
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

struct FeatList {
    float x[PH_MAX_FEAT], y[PH_MAX_FEAT], z[PH_MAX_FEAT];
    uint8_t type[PH_MAX_FEAT];
};

// sum over the features i of `other` of type t, ascending, of expf(-0.5 d2): fp32 terms, fp64 sum
__device__ __forceinline__ double feature_sum(const FeatList& other, int n_other, int t, float x, float y, float z) {
    double s = 0.0;
    for (int i = 0; i < n_other; ++i)
        if (other.type[i] == t) s += (double)expf(-0.5f * dist2(x, y, z, other.x[i], other.y[i], other.z[i]));
    return s;
}

__global__ __launch_bounds__(PH_MAXW) void k_pharm_score(const float* __restrict__ coords,
                                                         const int32_t* __restrict__ n_nodes,
                                                         const uint8_t* __restrict__ types,
                                                         const u64* __restrict__ ring_mask,
                                                         const int32_t* __restrict__ n_rings, int N, int W,
                                                         const float* __restrict__ ref_xyz,
                                                         const uint8_t* __restrict__ ref_type, int F,
                                                         const double* __restrict__ o_rr_in,
                                                         double* __restrict__ o_rm_out, double* __restrict__ o_mm_out,
                                                         float* __restrict__ tanimoto_out,
                                                         int32_t* __restrict__ matches_out,
                                                         double* __restrict__ per_type_out) {
    __shared__ FeatList ref, cand;
    __shared__ double sum_rm[PH_MAX_FEAT], sum_mm[PH_MAX_FEAT];
    __shared__ double part_rm[6], part_mm[6];
    __shared__ float ax[PH_MAXW], ay[PH_MAXW], az[PH_MAXW];
    __shared__ int offset[PH_MAXW];

    const int b = blockIdx.x, a = threadIdx.x;
    for (int i = a; i < F; i += PH_MAXW) {
        ref.x[i] = ref_xyz[3 * i], ref.y[i] = ref_xyz[3 * i + 1], ref.z[i] = ref_xyz[3 * i + 2];
        ref.type[i] = ref_type[i];
    }
    int n_cand = 0;
    bool bad = false;
    if (coords == nullptr) {                     // the reference against itself
        __syncthreads();
        for (int i = a; i < F; i += PH_MAXW) {
            cand.x[i] = ref.x[i], cand.y[i] = ref.y[i], cand.z[i] = ref.z[i];
            cand.type[i] = ref.type[i];
        }
        n_cand = F;
    } else {
        const int n = min(max(n_nodes[b], 0), min(N, W));
        const bool real = a < n;
        const int rings_b = n_rings[b];
        const int nr = min(max(rings_b, 0), PH_MAX_RINGS);
        float x = 0.f, y = 0.f, zc = 0.f;
        int t = 0;
        if (real) {
            const float* p = coords + ((size_t)b * N + a) * 3;
            x = p[0], y = p[1], zc = p[2];
            t = types[(size_t)b * W + a] & 31;
        }
        ax[a] = x, ay[a] = y, az[a] = zc;
        const bool finite = isfinite(x) && isfinite(y) && isfinite(zc);
        bad = __ballot(real && !finite) != 0ull || rings_b > PH_MAX_RINGS;
        // this atom's entries start behind those of the atoms below it
        const int mine = __popc(t);
        int incl = mine;
        for (int off = 1; off < PH_MAXW; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (a >= off) incl += v;
        }
        const int n_atom_feat = __shfl(incl, PH_MAXW - 1);
        int at = incl - mine;
        for (int k = 0; k < 5; ++k)
            if (t >> k & 1) {
                cand.x[at] = x, cand.y[at] = y, cand.z[at] = zc;
                cand.type[at] = (uint8_t)k;
                ++at;
            }
        __syncthreads();
        // rings in list order; a mask is read over the real atoms only, an empty one is no feature
        const u64 live = low_bits(n);
        u64 m = (a < nr) ? (ring_mask[(size_t)b * PH_MAX_RINGS + a] & live) : 0ull;
        const u64 has = __ballot(m != 0ull);
        if (m != 0ull) {
            const int slot = n_atom_feat + __popcll(has & low_bits(a));
            const float cnt = (float)__popcll(m);
            float sx = 0.f, sy = 0.f, sz = 0.f;
            for (; m != 0ull; m &= m - 1ull) {
                const int k = low_bit(m);
                sx = __fadd_rn(sx, ax[k]), sy = __fadd_rn(sy, ay[k]), sz = __fadd_rn(sz, az[k]);
            }
            cand.x[slot] = __fdiv_rn(sx, cnt), cand.y[slot] = __fdiv_rn(sy, cnt), cand.z[slot] = __fdiv_rn(sz, cnt);
            cand.type[slot] = (uint8_t)PH_T_RING;
        }
        n_cand = n_atom_feat + __popcll(has);
    }
    __syncthreads();

    for (int j = a; j < n_cand; j += PH_MAXW) {
        const int t = cand.type[j];
        const float x = cand.x[j], y = cand.y[j], zc = cand.z[j];
        sum_rm[j] = feature_sum(ref, F, t, x, y, zc);
        sum_mm[j] = feature_sum(cand, n_cand, t, x, y, zc);
    }
    // reference features with a candidate feature of their type within 1.5 A
    int hit = 0;
    for (int i = a; i < F; i += PH_MAXW) {
        const int t = ref.type[i];
        bool near = false;
        for (int j = 0; j < n_cand; ++j)
            near = near || (cand.type[j] == t &&
                            dist2(ref.x[i], ref.y[i], ref.z[i], cand.x[j], cand.y[j], cand.z[j]) <= 2.25f);
        hit += near ? 1 : 0;
    }
    hit = wave_sum(hit);
    __syncthreads();
    if (a < 6) {
        double rm = 0.0, mm = 0.0;
        for (int j = 0; j < n_cand; ++j)
            if (cand.type[j] == a) rm += sum_rm[j], mm += sum_mm[j];
        part_rm[a] = rm, part_mm[a] = mm;
    }
    __syncthreads();
    if (a == 0) {
        double rm = 0.0, mm = 0.0;
        for (int t = 0; t < 6; ++t) rm += part_rm[t], mm += part_mm[t];
        const double nan = __builtin_nan("");
        const double rr = o_rr_in != nullptr ? o_rr_in[0] : mm;
        o_rm_out[b] = bad ? nan : rm;
        o_mm_out[b] = bad ? nan : mm;
        tanimoto_out[b] = bad ? __builtin_nanf("") : (float)(rm / (rr + mm - rm));
        matches_out[b] = bad ? -1 : hit;
    }
    if (per_type_out != nullptr && a < 6) per_type_out[(size_t)b * 6 + a] = bad ? __builtin_nan("") : part_rm[a];
}

}  // namespace

extern "C" int mcg_pharm_perceive(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                                  uint8_t* types_out, int32_t* n_rings_out, uint64_t* ring_mask_out, void* stream) {
    if (!z || !bonds || !n_nodes_dev || !types_out || !n_rings_out || !ring_mask_out || B < 0 || W < 1 || W > PH_MAXW) {
        mcg_set_error("mcg_pharm_perceive: bad arguments (non-null z, bonds, n_nodes, types_out, n_rings_out and "
                      "ring_mask_out, B >= 0, 1 <= W <= %d)", PH_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_pharm_perceive, dim3((unsigned)B), dim3(PH_MAXW), 0, (hipStream_t)stream, z, bonds, n_nodes_dev,
                       W, types_out, n_rings_out, reinterpret_cast<u64*>(ring_mask_out));
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_pharm_score(const float* coords, const int32_t* n_nodes_dev, const uint8_t* types,
                               const uint64_t* ring_mask, const int32_t* n_rings, int B, int N, int W,
                               const float* ref_xyz, const uint8_t* ref_type, int F, const double* o_rr, double* o_rm,
                               double* o_mm, float* tanimoto, int32_t* matches, double* per_type, void* stream) {
    const bool self = coords == nullptr;
    const bool rows_ok = self ? (B == 0 || B == 1) : (n_nodes_dev && types && ring_mask && n_rings && N >= 1 &&
                                                      N <= PH_MAXW && W >= 1 && W <= PH_MAXW);
    if (!rows_ok || !ref_xyz || !ref_type || !o_rm || !o_mm || !tanimoto || !matches || B < 0 || F < 1 ||
        F > PH_MAX_FEAT) {
        mcg_set_error("mcg_pharm_score: bad arguments (non-null n_nodes, types, ring_mask, n_rings, ref_xyz, ref_type, "
                      "o_rm, o_mm, tanimoto and matches, B >= 0, 1 <= N, W <= %d, 1 <= F <= %d; coords NULL: the "
                      "reference against itself, B <= 1)", PH_MAXW, PH_MAX_FEAT);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_pharm_score, dim3((unsigned)B), dim3(PH_MAXW), 0, (hipStream_t)stream, coords, n_nodes_dev, types,
                       reinterpret_cast<const u64*>(ring_mask), n_rings, N, W, ref_xyz, ref_type, F, o_rr, o_rm, o_mm,
                       tanimoto, matches, per_type);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
