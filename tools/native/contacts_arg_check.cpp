// Host-only driver of `mcg_receptor_contacts`' argument checking (csrc/mcg_contacts.hip), built with AddressSanitizer +
// UBSan on the host side by `make -C ml_conformer_generator_amd/csrc asan_contacts` and run on the CPU: every call below
// must be refused with MCG_ERR_ARG before anything is launched or dereferenced.  The exit code is the number of calls that
// were not (sanitizer reports abort the process on their own).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/mlconfgen_hip_contacts.h"

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
    const int32_t* yg;
    int R;
    const float* sph;
    const int32_t* rg;
    const uint8_t* rk;
    int K, mask;
    int32_t* groups;
    uint8_t* kinds;
    int32_t* n_groups;
    uint8_t* atom_kinds;
    int32_t *status, *counts;
};

static int call(const Args& a) {
    g_err[0] = 0;
    return mcg_receptor_contacts(a.x, a.r, a.t, a.nn, a.B, a.N, a.y, a.yt, a.yg, a.R, a.sph, a.rg, a.rk, a.K, a.mask,
                                 a.groups, a.kinds, a.n_groups, a.atom_kinds, a.status, a.counts, nullptr);
}

int main() {
    static float buf[64];                     // never read: every call fails its check first
    static uint8_t bytes[16];
    static int32_t n[4];
    const Args ok = {buf, buf, bytes, n, 3, 27, buf, bytes, n, 100, buf, n, bytes, 2, 14, n, bytes, n, bytes, n, n};
    int n_calls = 0, n_bad = 0;
    auto refused = [&](Args a, const char* what) {
        ++n_calls;
        const int rc = call(a);
        if (rc != 1 || !strstr(g_err, "mcg_receptor_contacts")) {
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
    a = ok; a.yg = nullptr; refused(a, "rec_group NULL");
    a = ok; a.groups = nullptr; refused(a, "groups NULL");
    a = ok; a.kinds = nullptr; refused(a, "kinds NULL");
    a = ok; a.n_groups = nullptr; refused(a, "n_groups NULL");
    a = ok; a.atom_kinds = nullptr; refused(a, "atom_kinds NULL");
    a = ok; a.status = nullptr; refused(a, "status NULL");
    a = ok; a.rg = nullptr; refused(a, "ref_group NULL with counts and K_ref > 0");
    a = ok; a.rk = nullptr; refused(a, "ref_kinds NULL with counts and K_ref > 0");
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
    a = ok; a.K = -1; refused(a, "K_ref < 0");
    a = ok; a.K = MCG_CONTACT_MAX_GROUPS + 1; refused(a, "K_ref 257");
    a = ok; a.K = std::numeric_limits<int>::max(); a.counts = nullptr; refused(a, "K_ref INT_MAX without counts");
    a = ok; a.mask = -1; refused(a, "kinds_mask < 0");
    a = ok; a.mask = MCG_CONTACT_ALL_KINDS + 1; refused(a, "kinds_mask 16");
    a = ok; a.sph = nullptr; a.counts = nullptr; a.B = 0; refused(a, "B 0 without spheres and counts");
    printf("contacts_arg_check: %d calls, %d not refused\n", n_calls, n_bad);
    return n_bad;
}
