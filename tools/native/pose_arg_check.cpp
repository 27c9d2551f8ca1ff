// Host-only driver of `mcg_receptor_optimise`'s argument checking (csrc/mcg_pose_optimise.hip), built with
// AddressSanitizer + UBSan on the host side by `make -C ml_conformer_generator_amd/csrc asan_pose` and run on the CPU:
// every call below must be refused with MCG_ERR_ARG before anything is launched or dereferenced.  The exit code is the
// number of calls that were not (sanitizer reports abort the process on their own).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/mlconfgen_hip.h"

static char g_err[512];
extern "C" void mcg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct Args {
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
    float *coords, *xform, *stats, *grad, *trace;
};

static int call(const Args& a) {
    g_err[0] = 0;
    return mcg_receptor_optimise(a.x, a.r, a.t, a.nn, a.B, a.N, a.y, a.yt, a.R, a.sph, a.steps, a.max_shift, a.coords,
                                 a.xform, a.stats, a.grad, a.trace, nullptr);
}

int main() {
    static float buf[64];                     // never read: every call fails its check first
    static uint8_t bytes[16];
    static int32_t n[4];
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const Args ok = {buf, buf, bytes, n, 3, 27, buf, bytes, 100, buf, 64, 2.0f, buf, buf, buf, buf, buf};
    int n_calls = 0, n_bad = 0;
    auto refused = [&](Args a, const char* what) {
        ++n_calls;
        const int rc = call(a);
        if (rc != 1 || !strstr(g_err, "mcg_receptor_optimise")) {
            fprintf(stderr, "not refused: %s (rc %d, '%s')\n", what, rc, g_err);
            ++n_bad;
        }
    };
    Args a;
    a = ok; a.x = nullptr; refused(a, "lig_xyz NULL");
    a = ok; a.r = nullptr; refused(a, "lig_radius NULL");
    a = ok; a.t = nullptr; refused(a, "lig_type NULL");
    a = ok; a.nn = nullptr; refused(a, "n_nodes NULL");
    a = ok; a.y = nullptr; refused(a, "rec_xyzr NULL");
    a = ok; a.yt = nullptr; refused(a, "rec_type NULL");
    a = ok; a.coords = nullptr; refused(a, "coords_out NULL");
    a = ok; a.xform = nullptr; refused(a, "xform_out NULL");
    a = ok; a.stats = nullptr; refused(a, "stats_out NULL");
    a = ok; a.B = 0; refused(a, "B 0");
    a = ok; a.B = -7; refused(a, "B < 0");
    a = ok; a.B = MCG_RECEPTOR_MAX_B + 1; refused(a, "B too large");
    a = ok; a.B = std::numeric_limits<int>::max(); refused(a, "B INT_MAX");
    a = ok; a.N = 0; refused(a, "N 0");
    a = ok; a.N = 65; refused(a, "N 65");
    a = ok; a.N = std::numeric_limits<int>::min(); refused(a, "N INT_MIN");
    a = ok; a.R = 0; refused(a, "R 0");
    a = ok; a.R = -1; refused(a, "R < 0");
    a = ok; a.R = MCG_RECEPTOR_MAX_ATOMS + 1; refused(a, "R too large");
    a = ok; a.R = std::numeric_limits<int>::max(); refused(a, "R INT_MAX");
    a = ok; a.steps = -1; refused(a, "steps < 0");
    a = ok; a.steps = 1025; refused(a, "steps 1025");
    a = ok; a.steps = std::numeric_limits<int>::max(); refused(a, "steps INT_MAX");
    a = ok; a.max_shift = -0.5f; refused(a, "max_shift < 0");
    a = ok; a.max_shift = inf; refused(a, "max_shift inf");
    a = ok; a.max_shift = -inf; refused(a, "max_shift -inf");
    a = ok; a.max_shift = nan; refused(a, "max_shift NaN");
    a = ok; a.sph = nullptr; a.grad = nullptr; a.trace = nullptr; a.B = 0; refused(a, "B 0 without the optional buffers");
    printf("pose_arg_check: %d calls, %d not refused\n", n_calls, n_bad);
    return n_bad;
}
