// Host-only driver of the argument checking of `mcg_ring_scaffold` and `mcg_induced_subgraph` (csrc/mcg_scaffold.hip),
// built with AddressSanitizer + UBSan on the host side by `make -C ml_conformer_generator_amd/csrc asan_scaffold` and run on
// the CPU: every call below must be refused with MCG_ERR_ARG before anything is launched or dereferenced, and B = 0 must
// return MCG_OK without a launch.  The exit code is the number of calls that did otherwise (sanitizer reports abort the
// process on their own).
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

struct Rings {
    const int32_t* z;
    const int8_t* bonds;
    const int32_t* nn;
    int B, W;
    uint64_t* ring_nb;
    int32_t *ring_size, *ring_system;
    uint64_t* masks;
    int32_t* counts;
};

struct Sub {
    const int32_t* z;
    const int8_t* bonds;
    const int32_t* nn;
    const uint64_t* mask;
    int mode, B, W;
    int32_t* z_out;
    int8_t* bonds_out;
    int32_t *n_out, *map_out;
};

static int call(const Rings& a) {
    g_err[0] = 0;
    return mcg_ring_scaffold(a.z, a.bonds, a.nn, a.B, a.W, a.ring_nb, a.ring_size, a.ring_system, a.masks, a.counts, nullptr);
}

static int call(const Sub& a) {
    g_err[0] = 0;
    return mcg_induced_subgraph(a.z, a.bonds, a.nn, a.mask, a.mode, a.B, a.W, a.z_out, a.bonds_out, a.n_out, a.map_out,
                                nullptr);
}

static int n_calls = 0, n_bad = 0;

template <class A>
static void refused(const A& a, const char* who, const char* what) {
    ++n_calls;
    const int rc = call(a);
    if (rc != 1 || !strstr(g_err, who)) {
        fprintf(stderr, "not refused: %s %s (rc %d, '%s')\n", who, what, rc, g_err);
        ++n_bad;
    }
}

template <class A>
static void accepted_empty(A a, const char* who) {
    ++n_calls;
    a.B = 0;
    const int rc = call(a);
    if (rc != 0 || g_err[0]) {
        fprintf(stderr, "B = 0 did not return MCG_OK: %s (rc %d, '%s')\n", who, rc, g_err);
        ++n_bad;
    }
}

// the refusals both entries share: B and W out of range
template <class A>
static void sizes(const A& ok, const char* who) {
    const int big = std::numeric_limits<int>::max(), small = std::numeric_limits<int>::min();
    A a;
    a = ok; a.B = -1; refused(a, who, "B < 0");
    a = ok; a.B = MCG_SCAFFOLD_MAX_B + 1; refused(a, who, "B too large");
    a = ok; a.B = big; refused(a, who, "B INT_MAX");
    a = ok; a.B = small; refused(a, who, "B INT_MIN");
    a = ok; a.W = 0; refused(a, who, "W 0");
    a = ok; a.W = MCG_SCAFFOLD_MAX_ATOMS + 1; refused(a, who, "W 65");
    a = ok; a.W = big; refused(a, who, "W INT_MAX");
    a = ok; a.W = small; refused(a, who, "W INT_MIN");
    accepted_empty(ok, who);
}

int main() {
    static int32_t i32[8];                    // never read: every call fails its check first, or has B = 0
    static int8_t i8[8];
    static uint64_t u64[8];
    const int big = std::numeric_limits<int>::max(), small = std::numeric_limits<int>::min();

    const char* who = "mcg_ring_scaffold";
    const Rings ok = {i32, i8, i32, 3, 27, u64, i32, i32, u64, i32};
    Rings a;
    a = ok; a.z = nullptr; refused(a, who, "z NULL");
    a = ok; a.bonds = nullptr; refused(a, who, "bonds NULL");
    a = ok; a.nn = nullptr; refused(a, who, "n_nodes NULL");
    a = ok; a.ring_nb = nullptr; refused(a, who, "ring_nb_out NULL");
    a = ok; a.ring_size = nullptr; refused(a, who, "ring_size_out NULL");
    a = ok; a.ring_system = nullptr; refused(a, who, "ring_system_out NULL");
    a = ok; a.masks = nullptr; refused(a, who, "masks_out NULL");
    a = ok; a.counts = nullptr; refused(a, who, "counts_out NULL");
    sizes(ok, who);

    who = "mcg_induced_subgraph";
    const Sub sok = {i32, i8, i32, u64, 0, 3, 27, i32, i8, i32, i32};
    Sub s;
    s = sok; s.z = nullptr; refused(s, who, "z NULL");
    s = sok; s.bonds = nullptr; refused(s, who, "bonds NULL");
    s = sok; s.nn = nullptr; refused(s, who, "n_nodes NULL");
    s = sok; s.mask = nullptr; refused(s, who, "mask NULL");
    s = sok; s.z_out = nullptr; refused(s, who, "z_out NULL");
    s = sok; s.bonds_out = nullptr; refused(s, who, "bonds_out NULL");
    s = sok; s.n_out = nullptr; refused(s, who, "n_out NULL");
    s = sok; s.map_out = nullptr; refused(s, who, "map_out NULL");
    s = sok; s.mode = -1; refused(s, who, "mode -1");
    s = sok; s.mode = 2; refused(s, who, "mode 2");
    s = sok; s.mode = big; refused(s, who, "mode INT_MAX");
    s = sok; s.mode = small; refused(s, who, "mode INT_MIN");
    sizes(sok, who);
    s = sok; s.mode = 1;
    accepted_empty(s, who);

    printf("scaffold_arg_check: %d calls, %d wrong\n", n_calls, n_bad);
    return n_bad;
}
