// Host-only driver of the argument checking of `mcg_pose_starts` and `mcg_pose_search_select`
// (csrc/mcg_pose_search.hip), built with AddressSanitizer + UBSan on the host side by
// `make -C ml_conformer_generator_amd/csrc asan_search` and run on the CPU: every call below must be refused with
// MCG_ERR_ARG before anything is launched or dereferenced.  The exit code is the number of calls that were not
// (sanitizer reports abort the process on their own).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/mlconfgen_hip_search.h"

static char g_err[512];
extern "C" void mcg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct Starts {
    const float* x;
    const int32_t* nn;
    int B, N;
    const int32_t* atoms;
    const uint64_t* side;
    const int32_t* nt;
    const int64_t* ids;
    uint64_t seed;
    int S;
    float spread, max_turn;
    float *xyz, *xform, *angles, *params;
};

struct Select {
    const float *wc, *wx, *ws, *wa, *sx, *sa, *x;
    const int32_t* nn;
    int B, N, S;
    float *coords, *xform, *stats, *angles;
    int32_t* best;
    float* scores;
};

static int call(const Starts& a) {
    g_err[0] = 0;
    return mcg_pose_starts(a.x, a.nn, a.B, a.N, a.atoms, a.side, a.nt, a.ids, a.seed, a.S, a.spread, a.max_turn, a.xyz,
                           a.xform, a.angles, a.params, nullptr);
}

static int call(const Select& a) {
    g_err[0] = 0;
    return mcg_pose_search_select(a.wc, a.wx, a.ws, a.wa, a.sx, a.sa, a.x, a.nn, a.B, a.N, a.S, a.coords, a.xform, a.stats,
                                  a.angles, a.best, a.scores, nullptr);
}

int main() {
    static float buf[64];                     // never read: every call fails its check first
    static int32_t n[4];
    static int64_t ids[4];
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
    const Starts sok = {buf, n, 3, 27, n, masks, n, ids, 7u, 8, 2.0f, 3.0f, buf, buf, buf, buf};
    const char* se = "mcg_pose_starts";
    Starts s;
    s = sok; s.x = nullptr; refused(s, se, "lig_xyz NULL");
    s = sok; s.nn = nullptr; refused(s, se, "n_nodes NULL");
    s = sok; s.atoms = nullptr; refused(s, se, "torsion_atoms NULL");
    s = sok; s.side = nullptr; refused(s, se, "side_mask NULL");
    s = sok; s.nt = nullptr; refused(s, se, "n_torsions NULL");
    s = sok; s.ids = nullptr; refused(s, se, "sample_ids NULL");
    s = sok; s.xyz = nullptr; refused(s, se, "start_xyz NULL");
    s = sok; s.xform = nullptr; refused(s, se, "start_xform NULL");
    s = sok; s.angles = nullptr; refused(s, se, "start_angles NULL");
    s = sok; s.B = 0; refused(s, se, "B 0");
    s = sok; s.B = -7; refused(s, se, "B < 0");
    s = sok; s.B = MCG_RECEPTOR_MAX_B + 1; refused(s, se, "B too large");
    s = sok; s.B = imax; refused(s, se, "B INT_MAX");
    s = sok; s.N = 0; refused(s, se, "N 0");
    s = sok; s.N = 65; refused(s, se, "N 65");
    s = sok; s.N = imin; refused(s, se, "N INT_MIN");
    s = sok; s.S = 0; refused(s, se, "S 0");
    s = sok; s.S = MCG_SEARCH_MAX_STARTS + 1; refused(s, se, "S 65");
    s = sok; s.S = imin; refused(s, se, "S INT_MIN");
    s = sok; s.S = imax; refused(s, se, "S INT_MAX");
    s = sok; s.spread = -0.5f; refused(s, se, "spread < 0");
    s = sok; s.spread = inf; refused(s, se, "spread inf");
    s = sok; s.spread = nan; refused(s, se, "spread NaN");
    s = sok; s.max_turn = -0.1f; refused(s, se, "max_turn < 0");
    s = sok; s.max_turn = 3.2f; refused(s, se, "max_turn > pi");
    s = sok; s.max_turn = inf; refused(s, se, "max_turn inf");
    s = sok; s.max_turn = nan; refused(s, se, "max_turn NaN");
    s = sok; s.params = nullptr; s.B = 0; refused(s, se, "B 0 without the optional buffer");

    const Select cok = {buf, buf, buf, buf, buf, buf, buf, n, 3, 27, 8, buf, buf, buf, buf, n, buf};
    const char* ce = "mcg_pose_search_select";
    Select c;
    c = cok; c.wc = nullptr; refused(c, ce, "walk_coords NULL");
    c = cok; c.wx = nullptr; refused(c, ce, "walk_xform NULL");
    c = cok; c.ws = nullptr; refused(c, ce, "walk_stats NULL");
    c = cok; c.wa = nullptr; refused(c, ce, "walk_angles NULL");
    c = cok; c.sx = nullptr; refused(c, ce, "start_xform NULL");
    c = cok; c.sa = nullptr; refused(c, ce, "start_angles NULL");
    c = cok; c.x = nullptr; refused(c, ce, "lig_xyz NULL");
    c = cok; c.nn = nullptr; refused(c, ce, "n_nodes NULL");
    c = cok; c.coords = nullptr; refused(c, ce, "coords_out NULL");
    c = cok; c.xform = nullptr; refused(c, ce, "xform_out NULL");
    c = cok; c.stats = nullptr; refused(c, ce, "stats_out NULL");
    c = cok; c.angles = nullptr; refused(c, ce, "angles_out NULL");
    c = cok; c.best = nullptr; refused(c, ce, "best_start NULL");
    c = cok; c.scores = nullptr; refused(c, ce, "start_scores NULL");
    c = cok; c.B = 0; refused(c, ce, "B 0");
    c = cok; c.B = MCG_RECEPTOR_MAX_B + 1; refused(c, ce, "B too large");
    c = cok; c.B = imin; refused(c, ce, "B INT_MIN");
    c = cok; c.N = 0; refused(c, ce, "N 0");
    c = cok; c.N = 65; refused(c, ce, "N 65");
    c = cok; c.N = imax; refused(c, ce, "N INT_MAX");
    c = cok; c.S = 0; refused(c, ce, "S 0");
    c = cok; c.S = MCG_SEARCH_MAX_STARTS + 1; refused(c, ce, "S 65");
    c = cok; c.S = imax; refused(c, ce, "S INT_MAX");
    printf("search_arg_check: %d calls, %d not refused\n", n_calls, n_bad);
    return n_bad;
}
