// Host-only driver of the argument checking of `mcg_torsion_tree` and `mcg_receptor_optimise_flex`
// (csrc/mcg_pose_flex.hip), built with AddressSanitizer + UBSan on the host side by
// `make -C ml_conformer_generator_amd/csrc asan_flex` and run on the CPU: every call below must be refused with
// MCG_ERR_ARG before anything is launched or dereferenced.  The exit code is the number of calls that were not
// (sanitizer reports abort the process on their own).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/mlconfgen_hip_flex.h"

static char g_err[512];
extern "C" void mcg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct Tree {
    const int32_t* z;
    const int8_t* bonds;
    const int32_t* nn;
    int B, W;
    int32_t* atoms;
    uint64_t *side, *near;
    int32_t* counts;
};

struct Walk {
    const float *x, *r;
    const uint8_t* t;
    const int32_t* nn;
    int B, N;
    const float* y;
    const uint8_t* yt;
    int R;
    const float* sph;
    int steps;
    float max_shift;
    const float* clash;
    const int32_t* atoms;
    const uint64_t *side, *near;
    const int32_t* nt;
    float *coords, *xform, *stats, *angles, *grad, *trace;
};

static int call(const Tree& a) {
    g_err[0] = 0;
    return mcg_torsion_tree(a.z, a.bonds, a.nn, a.B, a.W, a.atoms, a.side, a.near, a.counts, nullptr);
}

static int call(const Walk& a) {
    g_err[0] = 0;
    return mcg_receptor_optimise_flex(a.x, a.r, a.t, a.nn, a.B, a.N, a.y, a.yt, a.R, a.sph, a.steps, a.max_shift, a.clash,
                                      a.atoms, a.side, a.near, a.nt, a.coords, a.xform, a.stats, a.angles, a.grad, a.trace,
                                      nullptr);
}

int main() {
    static float buf[64];                     // never read: every call fails its check first
    static uint8_t bytes[16];
    static int8_t codes[16];
    static int32_t n[4];
    static uint64_t masks[4];
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    int n_calls = 0, n_bad = 0;
    auto refused = [&](auto a, const char* entry, const char* what) {
        ++n_calls;
        const int rc = call(a);
        if (rc != 1 || !strstr(g_err, entry)) {
            fprintf(stderr, "not refused: %s: %s (rc %d, '%s')\n", entry, what, rc, g_err);
            ++n_bad;
        }
    };
    const Tree tok = {n, codes, n, 3, 27, n, masks, masks, n};
    const char* te = "mcg_torsion_tree";
    Tree t;
    t = tok; t.z = nullptr; refused(t, te, "z NULL");
    t = tok; t.bonds = nullptr; refused(t, te, "bonds NULL");
    t = tok; t.nn = nullptr; refused(t, te, "n_nodes NULL");
    t = tok; t.atoms = nullptr; refused(t, te, "torsion_atoms NULL");
    t = tok; t.side = nullptr; refused(t, te, "side_mask NULL");
    t = tok; t.near = nullptr; refused(t, te, "near_mask NULL");
    t = tok; t.counts = nullptr; refused(t, te, "counts NULL");
    t = tok; t.B = -1; refused(t, te, "B < 0");
    t = tok; t.B = MCG_FLEX_MAX_B + 1; refused(t, te, "B too large");
    t = tok; t.B = imax; refused(t, te, "B INT_MAX");
    t = tok; t.W = 0; refused(t, te, "W 0");
    t = tok; t.W = MCG_FLEX_MAX_ATOMS + 1; refused(t, te, "W 65");
    t = tok; t.W = imin; refused(t, te, "W INT_MIN");
    t = tok; t.W = imax; refused(t, te, "W INT_MAX");
    ++n_calls;
    t = tok; t.B = 0;                         // B = 0 launches nothing and is no error
    if (call(t) != 0) {
        fprintf(stderr, "mcg_torsion_tree: B = 0 was refused\n");
        ++n_bad;
    }

    const Walk wok = {buf, buf, bytes, n, 3, 27, buf, bytes, 100, buf, 64, 2.0f, buf, n, masks, masks, n,
                      buf, buf, buf, buf, buf, buf};
    const char* we = "mcg_receptor_optimise_flex";
    Walk a;
    a = wok; a.x = nullptr; refused(a, we, "lig_xyz NULL");
    a = wok; a.r = nullptr; refused(a, we, "lig_radius NULL");
    a = wok; a.t = nullptr; refused(a, we, "lig_type NULL");
    a = wok; a.nn = nullptr; refused(a, we, "n_nodes NULL");
    a = wok; a.y = nullptr; refused(a, we, "rec_xyzr NULL");
    a = wok; a.yt = nullptr; refused(a, we, "rec_type NULL");
    a = wok; a.clash = nullptr; refused(a, we, "clash_radius NULL");
    a = wok; a.atoms = nullptr; refused(a, we, "torsion_atoms NULL");
    a = wok; a.side = nullptr; refused(a, we, "side_mask NULL");
    a = wok; a.near = nullptr; refused(a, we, "near_mask NULL");
    a = wok; a.nt = nullptr; refused(a, we, "n_torsions NULL");
    a = wok; a.coords = nullptr; refused(a, we, "coords_out NULL");
    a = wok; a.xform = nullptr; refused(a, we, "xform_out NULL");
    a = wok; a.stats = nullptr; refused(a, we, "stats_out NULL");
    a = wok; a.angles = nullptr; refused(a, we, "angles_out NULL");
    a = wok; a.B = 0; refused(a, we, "B 0");
    a = wok; a.B = -7; refused(a, we, "B < 0");
    a = wok; a.B = MCG_RECEPTOR_MAX_B + 1; refused(a, we, "B too large");
    a = wok; a.B = imax; refused(a, we, "B INT_MAX");
    a = wok; a.N = 0; refused(a, we, "N 0");
    a = wok; a.N = 65; refused(a, we, "N 65");
    a = wok; a.N = imin; refused(a, we, "N INT_MIN");
    a = wok; a.R = 0; refused(a, we, "R 0");
    a = wok; a.R = -1; refused(a, we, "R < 0");
    a = wok; a.R = MCG_RECEPTOR_MAX_ATOMS + 1; refused(a, we, "R too large");
    a = wok; a.R = imax; refused(a, we, "R INT_MAX");
    a = wok; a.steps = -1; refused(a, we, "steps < 0");
    a = wok; a.steps = 1025; refused(a, we, "steps 1025");
    a = wok; a.steps = imax; refused(a, we, "steps INT_MAX");
    a = wok; a.max_shift = -0.5f; refused(a, we, "max_shift < 0");
    a = wok; a.max_shift = inf; refused(a, we, "max_shift inf");
    a = wok; a.max_shift = -inf; refused(a, we, "max_shift -inf");
    a = wok; a.max_shift = nan; refused(a, we, "max_shift NaN");
    a = wok; a.sph = nullptr; a.grad = nullptr; a.trace = nullptr; a.B = 0; refused(a, we, "B 0 without the optional buffers");
    printf("flex_arg_check: %d calls, %d not refused\n", n_calls, n_bad);
    return n_bad;
}
