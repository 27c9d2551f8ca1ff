// Host-only driver of the argument checking of `mcg_charges_peoe` and `mcg_esp_overlap` (csrc/mcg_electrostatics.hip), built
// with AddressSanitizer + UBSan on the host side by `make -C ml_conformer_generator_amd/csrc asan_esp` and run on the CPU:
// every call below must be refused with MCG_ERR_ARG before anything is launched or dereferenced, and B = 0 must return
// MCG_OK without a launch.  The exit code is the number of calls that did otherwise (sanitizer reports abort the process
// on their own).
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

struct Charges {
    const int32_t* z;
    const int8_t* bonds;
    const int32_t* nn;
    const uint8_t* types;
    const uint64_t* rings;
    const int32_t* n_rings;
    int B, W;
    float *q, *qh;
    int32_t *nh, *status;
};

struct Overlap {
    const float *rx, *rq;
    int P;
    const float *x, *q;
    const int32_t* np;
    int B, PW;
    float mu;
    float *cross, *self, *t;
};

static int call(const Charges& a) {
    g_err[0] = 0;
    return mcg_charges_peoe(a.z, a.bonds, a.nn, a.types, a.rings, a.n_rings, a.B, a.W, a.q, a.qh, a.nh, a.status, nullptr);
}

static int call(const Overlap& a) {
    g_err[0] = 0;
    return mcg_esp_overlap(a.rx, a.rq, a.P, a.x, a.q, a.np, a.B, a.PW, a.mu, nullptr, a.cross, a.self, a.t, nullptr);
}

int main() {
    static float f[64];                       // never read: every call fails its check first, or has B = 0
    static int32_t i32[8];
    static int8_t i8[8];
    static uint8_t u8[8];
    static uint64_t u64[8];
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int big = std::numeric_limits<int>::max(), small = std::numeric_limits<int>::min();
    const Charges ok = {i32, i8, i32, u8, u64, i32, 3, 27, f, f, i32, i32};
    const Overlap fine = {f, f, 12, f, f, i32, 3, 40, 1.0f, f, f, f};
    int n_calls = 0, n_bad = 0;
    auto refused = [&](auto a, const char* who, const char* what) {
        ++n_calls;
        const int rc = call(a);
        if (rc != 1 || !strstr(g_err, who)) {
            fprintf(stderr, "not refused: %s %s (rc %d, '%s')\n", who, what, rc, g_err);
            ++n_bad;
        }
    };
    auto nothing = [&](auto a, const char* who) {
        ++n_calls;
        a.B = 0;
        const int rc = call(a);
        if (rc != 0 || g_err[0]) {
            fprintf(stderr, "B = 0 did not return MCG_OK: %s (rc %d, '%s')\n", who, rc, g_err);
            ++n_bad;
        }
    };
    const char* pe = "mcg_charges_peoe";
    Charges a;
    a = ok; a.z = nullptr; refused(a, pe, "z NULL");
    a = ok; a.bonds = nullptr; refused(a, pe, "bonds NULL");
    a = ok; a.nn = nullptr; refused(a, pe, "n_nodes NULL");
    a = ok; a.types = nullptr; refused(a, pe, "types NULL");
    a = ok; a.rings = nullptr; refused(a, pe, "ring_mask NULL");
    a = ok; a.n_rings = nullptr; refused(a, pe, "n_rings NULL");
    a = ok; a.q = nullptr; refused(a, pe, "q_out NULL");
    a = ok; a.qh = nullptr; refused(a, pe, "qh_out NULL");
    a = ok; a.nh = nullptr; refused(a, pe, "nh_out NULL");
    a = ok; a.status = nullptr; refused(a, pe, "status_out NULL");
    a = ok; a.B = -1; refused(a, pe, "B < 0");
    a = ok; a.B = MCG_CHARGES_MAX_B + 1; refused(a, pe, "B too large");
    a = ok; a.B = big; refused(a, pe, "B INT_MAX");
    a = ok; a.B = small; refused(a, pe, "B INT_MIN");
    a = ok; a.W = 0; refused(a, pe, "W 0");
    a = ok; a.W = MCG_CHARGES_MAX_ATOMS + 1; refused(a, pe, "W 65");
    a = ok; a.W = big; refused(a, pe, "W INT_MAX");
    a = ok; a.W = small; refused(a, pe, "W INT_MIN");
    nothing(ok, pe);

    const char* es = "mcg_esp_overlap";
    Overlap o;
    o = fine; o.rx = nullptr; refused(o, es, "ref_xyz NULL");
    o = fine; o.rq = nullptr; refused(o, es, "ref_q NULL");
    o = fine; o.x = nullptr; refused(o, es, "xyz NULL");
    o = fine; o.q = nullptr; refused(o, es, "q NULL");
    o = fine; o.np = nullptr; refused(o, es, "n_points NULL");
    o = fine; o.cross = nullptr; refused(o, es, "cross_out NULL");
    o = fine; o.self = nullptr; refused(o, es, "self_out NULL");
    o = fine; o.t = nullptr; refused(o, es, "tanimoto_out NULL");
    o = fine; o.B = -1; refused(o, es, "B < 0");
    o = fine; o.B = MCG_ESP_MAX_B + 1; refused(o, es, "B too large");
    o = fine; o.B = big; refused(o, es, "B INT_MAX");
    o = fine; o.P = 0; refused(o, es, "P 0");
    o = fine; o.P = MCG_ESP_MAX_POINTS + 1; refused(o, es, "P 257");
    o = fine; o.P = small; refused(o, es, "P INT_MIN");
    o = fine; o.PW = 0; refused(o, es, "PW 0");
    o = fine; o.PW = MCG_ESP_MAX_POINTS + 1; refused(o, es, "PW 257");
    o = fine; o.PW = big; refused(o, es, "PW INT_MAX");
    o = fine; o.mu = 0.f; refused(o, es, "mu 0");
    o = fine; o.mu = -1.f; refused(o, es, "mu < 0");
    o = fine; o.mu = nan; refused(o, es, "mu NaN");
    o = fine; o.mu = inf; refused(o, es, "mu inf");
    nothing(fine, es);
    printf("esp_arg_check: %d calls, %d wrong\n", n_calls, n_bad);
    return n_bad;
}
