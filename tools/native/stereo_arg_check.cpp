// Host-only driver of the argument checking of `mcg_stereo_order` (csrc/mcg_canonical.hip), built with AddressSanitizer +
// UBSan on the host side by `make -C ml_conformer_generator_amd/csrc asan_stereo` and run on the CPU: every call below
// must be refused with MCG_ERR_ARG before anything is launched or dereferenced, and B = 0 must return MCG_OK without a
// launch.  The exit code is the number of calls that did otherwise (sanitizer reports abort the process on their own).
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
    const float* coords;
    const int32_t* z;
    const int8_t* bonds;
    const int32_t* nn;
    int B, W;
    int32_t *order, *status, *leaves;
    uint64_t* key;
    int8_t* stereo;
    uint64_t* stereo_key;
    int32_t* counts;
};

static int call(const Args& a) {
    g_err[0] = 0;
    return mcg_stereo_order(a.coords, a.z, a.bonds, a.nn, a.B, a.W, a.order, a.status, a.leaves, a.key, a.stereo,
                            a.stereo_key, a.counts, nullptr);
}

int main() {
    static float f32[8];                      // never read: every call fails its check first, or has B = 0
    static int32_t i32[8];
    static int8_t i8[8];
    static uint64_t u64[8];
    const int big = std::numeric_limits<int>::max(), small = std::numeric_limits<int>::min();
    const Args ok = {f32, i32, i8, i32, 3, 27, i32, i32, i32, u64, i8, u64, i32};
    const char* who = "mcg_stereo_order";
    int n_calls = 0, n_bad = 0;
    auto refused = [&](const Args& a, const char* what) {
        ++n_calls;
        const int rc = call(a);
        if (rc != 1 || !strstr(g_err, who)) {
            fprintf(stderr, "not refused: %s %s (rc %d, '%s')\n", who, what, rc, g_err);
            ++n_bad;
        }
    };
    Args a;
    a = ok; a.coords = nullptr; refused(a, "coords NULL");
    a = ok; a.z = nullptr; refused(a, "z NULL");
    a = ok; a.bonds = nullptr; refused(a, "bonds NULL");
    a = ok; a.nn = nullptr; refused(a, "n_nodes NULL");
    a = ok; a.order = nullptr; refused(a, "order_out NULL");
    a = ok; a.status = nullptr; refused(a, "status_out NULL");
    a = ok; a.leaves = nullptr; refused(a, "leaves_out NULL");
    a = ok; a.key = nullptr; refused(a, "key_out NULL");
    a = ok; a.stereo = nullptr; refused(a, "stereo_out NULL");
    a = ok; a.stereo_key = nullptr; refused(a, "stereo_key_out NULL");
    a = ok; a.counts = nullptr; refused(a, "counts_out NULL");
    a = ok; a.B = -1; refused(a, "B < 0");
    a = ok; a.B = MCG_CANONICAL_MAX_B + 1; refused(a, "B too large");
    a = ok; a.B = big; refused(a, "B INT_MAX");
    a = ok; a.B = small; refused(a, "B INT_MIN");
    a = ok; a.W = 0; refused(a, "W 0");
    a = ok; a.W = MCG_CANONICAL_MAX_ATOMS + 1; refused(a, "W 65");
    a = ok; a.W = big; refused(a, "W INT_MAX");
    a = ok; a.W = small; refused(a, "W INT_MIN");
    ++n_calls;
    a = ok; a.B = 0;
    const int rc = call(a);
    if (rc != 0 || g_err[0]) {
        fprintf(stderr, "B = 0 did not return MCG_OK: %s (rc %d, '%s')\n", who, rc, g_err);
        ++n_bad;
    }
    printf("stereo_arg_check: %d calls, %d wrong\n", n_calls, n_bad);
    return n_bad;
}
