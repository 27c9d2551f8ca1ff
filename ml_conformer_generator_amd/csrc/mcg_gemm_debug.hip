// mcg_debug_gemm / mcg_debug_gemm_pack (include/mlconfgen_hip.h): ONE node-GEMM launch on the caller's data through the real
// packers and launchers of mcg_gemm.h, with every contract of the kernels checked on the host first.  The kernel-level harness
// of tests/test_gemm_gpu.py drives it; nothing here is on a hot path.
#include "mcg_egnn_internal.h"
#include "mcg_gemm.h"

namespace {

constexpr int64_t kMaxFloats = (int64_t)1 << 29;      // 32-bit byte offsets inside the kernels

int n_tiles_of(int n_out) { return (n_out + 15) / 16; }

// false + error text (`what` names the failed contract)
bool refuse(const char* what) {
    mcg_set_error("mcg_debug_gemm: %s", what);
    return false;
}

// rows of a gathered A2 a kernel of `family` sums per output row (0: plain rows)
int gather_width(const mcg_gemm_desc& d) {
    if (!d.a2_rows) return 0;
    return d.family == MCG_GEMM_BF16 ? (d.a2_nsum > 2 ? 4 : 2) : d.a2_nsum;
}

// floats of a row the family's kernels read
int64_t row_reach(int family, int K) { return (family == MCG_GEMM_BF16 || family == MCG_GEMM_X6) ? 32 * (int64_t)mcg_kblocks16(K) : K; }

bool check_operand(const char* name, int family, int K, int ld, int64_t rows, int64_t floats) {
    static thread_local char msg[160];
    if (ld < K || ld % 4 != 0) {
        snprintf(msg, sizeof msg, "%s: leading dimension %d must be a multiple of 4 and >= K = %d", name, ld, K);
        return refuse(msg);
    }
    const int64_t need = (rows - 1) * ld + row_reach(family, K);
    if (floats < need || floats > kMaxFloats) {
        snprintf(msg, sizeof msg, "%s: the kernel reads %lld floats ((rows - 1) * ld + %lld per row), the buffer is stated as %lld (limit 2^29)",
                 name, (long long)need, (long long)row_reach(family, K), (long long)floats);
        return refuse(msg);
    }
    return true;
}

bool check_desc(const mcg_gemm_desc* dp, const mcg_gemm_ran* ran) {
    if (!dp || !ran) return refuse("null descriptor or result");
    const mcg_gemm_desc& d = *dp;
    for (int r : d.reserved)
        if (r != 0) return refuse("reserved fields must be zero");
    if (!d.w_host || !d.A1 || !d.C) return refuse("w_host, A1 and C are required");
    if (d.family < MCG_GEMM_F32 || d.family > MCG_GEMM_X6) return refuse("family must be MCG_GEMM_F32 .. MCG_GEMM_X6");
    if (d.act < MCG_ACT_NONE || d.act > MCG_ACT_RELU) return refuse("act must be 0 (none), 1 (SiLU) or 2 (ReLU)");
    if (d.M < 1 || d.M > (1 << 20)) return refuse("M must be in 1 .. 2^20");
    if (d.n_out < 1 || d.n_out > (1 << 16)) return refuse("n_out must be in 1 .. 2^16 (n_tiles >= 1)");
    const int n_tiles = n_tiles_of(d.n_out);
    if (d.n_store < 1 || d.n_store > 16 * n_tiles) return refuse("n_store must be in 1 .. 16 * n_tiles");
    if (d.K1 < 4 || d.K1 % 4 != 0 || d.K1 > (1 << 16)) return refuse("K1 must be a multiple of 4 in 4 .. 2^16 (K1 % 4 == 0)");
    if (d.K2 < 0 || d.K2 % 4 != 0 || d.K2 > (1 << 16)) return refuse("K2 must be a multiple of 4 in 0 .. 2^16 (K2 % 4 == 0)");
    if ((d.K2 > 0) != (d.A2 != nullptr)) return refuse("A2 must be set exactly when K2 > 0 (a gather needs K2 > 0)");
    // gather
    if (d.a2_rows) {
        if (d.K2 <= 0) return refuse("a gather (a2_rows) needs K2 > 0");
        if (d.family != MCG_GEMM_F32ROWS16 && d.family != MCG_GEMM_BF16) return refuse("only MCG_GEMM_F32ROWS16 and MCG_GEMM_BF16 have gathering kernels");
        if (d.a2_nsum < 2 || d.a2_nsum > 4) return refuse("a2_nsum must be 2, 3 or 4 with a2_rows");
        if (d.a2_src_rows < 1) return refuse("a2_src_rows (rows of the gathered A2) must be >= 1");
    } else if (d.a2_nsum != 0 || d.a2_src_rows != 0) {
        return refuse("a2_nsum and a2_src_rows must be 0 without a2_rows");
    }
    // the launchers' own refusals, by the launchers' own predicate
    {
        McgGemmArgs a{};
        a.resid = d.resid; a.n_store = d.n_store; a.c_blocked = d.c_blocked; a.n_tiles = n_tiles;
        if (mcg_gemm_out_of_contract(a, d.family == MCG_GEMM_F32 || d.family == MCG_GEMM_BF16))
            return refuse(!(d.resid && d.n_store % 4 != 0) ? "c_blocked is implemented by the MCG_GEMM_F32 and MCG_GEMM_BF16 kernels only, for n_tiles == 54 (two parts of 27 column tiles)"
                                      : "a residual needs n_store % 4 == 0 (the kernels drop it on a ragged last piece)");
    }
    // operands
    if (!check_operand("A1", d.family, d.K1, d.lda1, d.M, d.a1_floats)) return false;
    if (d.K2 > 0 && !check_operand("A2", d.family, d.K2, d.lda2, d.a2_rows ? d.a2_src_rows : d.M, d.a2_floats)) return false;
    if (d.resid) {
        if (d.ldr < d.n_store || d.ldr % 4 != 0) return refuse("ldr must be a multiple of 4 and >= n_store");
        if (d.resid_floats < (int64_t)(d.M - 1) * d.ldr + d.n_store || d.resid_floats > kMaxFloats) return refuse("resid_floats does not cover (M - 1) * ldr + n_store (limit 2^29)");
    }
    if (d.c_blocked != 0 && d.c_blocked != 1) return refuse("c_blocked must be 0 or 1");
    if (d.c_blocked) {
        if (d.c_floats < (int64_t)896 * d.M || d.c_floats > kMaxFloats) return refuse("c_floats does not cover the blocked layout, 896 * M floats (limit 2^29)");
    } else {
        if (d.ldc < d.n_store || d.ldc % 4 != 0) return refuse("ldc must be a multiple of 4 and >= n_store");
        if (d.c_floats < (int64_t)(d.M - 1) * d.ldc + d.n_store || d.c_floats > kMaxFloats) return refuse("c_floats does not cover (M - 1) * ldc + n_store (limit 2^29)");
    }
    // side job
    if (d.side_x || d.side_u || d.side_slots || d.side_M != 0 || d.side_u_rows != 0) {
        if (d.family == MCG_GEMM_X6) return refuse("the MCG_GEMM_X6 kernel carries no side job");
        if (!d.side_x || !d.side_u || !d.side_slots) return refuse("a side job needs side_x, side_u and side_slots");
        if (d.side_M < 1 || d.side_M > (1 << 20) || d.side_u_rows < 1 || d.side_u_rows > (1 << 24)) return refuse("a side job needs side_M >= 1 and side_u_rows >= 1");
    }
    // selection
    if (d.deep != 0 && d.deep != 1) return refuse("deep must be 0 or 1");
    if (d.family == MCG_GEMM_F32ROWS16) {
        const bool ok = d.mr == 1 ? (d.rn == 1 || d.rn == 2 || d.rn == 3 || d.rn == 6) : d.mr == 2 ? (d.rn == 2 || d.rn == 3) : false;
        if (!ok) return refuse("MCG_GEMM_F32ROWS16 tiles: mr 1 with rn 1, 2, 3 or 6, or mr 2 with rn 2 or 3");
        if (d.deep && !(d.mr == 1 && d.rn <= 2)) return refuse("deep only with mr 1 and rn 1 or 2");
    } else {
        if (d.rn < 0 || d.rn > 3) return refuse("rn must be 0 (the launcher's choice) .. 3");
        if (d.mr != 0 || d.deep != 0) return refuse("mr and deep belong to MCG_GEMM_F32ROWS16 only");
    }
    if (d.lds < 0 || d.lds > 2 || (d.lds != 0 && d.family != MCG_GEMM_BF16)) return refuse("lds must be 0 .. 2, and 0 outside MCG_GEMM_BF16");
    return true;
}

// segment 1 then segment 2 of W[n_out][K1 + K2], rows >= n_out zero, into `f` (pack4) or `h` (pack16 / pack16x3)
void pack_segments(int kind, const float* w, int n_out, int K1, int K2, std::vector<float>& f, std::vector<uint16_t>& h) {
    const int n_tiles = n_tiles_of(n_out), K = K1 + K2;
    for (int seg = 0; seg < 2; ++seg) {
        const int Ks = seg == 0 ? K1 : K2, k0 = seg == 0 ? 0 : K1;
        if (Ks <= 0) continue;
        auto value = [&](int n, int k) -> float { return n < n_out ? w[(size_t)n * K + k0 + k] : 0.f; };
        if (kind == MCG_GEMM_PACK4) mcg_pack_b4(f, Ks, n_tiles, value);
        else if (kind == MCG_GEMM_PACK16) mcg_pack_b16(h, Ks, n_tiles, value);
        else mcg_pack_b16x3(h, Ks, n_tiles, value);
    }
}

// device blocks of one call, returned to the pool when it ends (after the stream has been synchronised)
struct Blocks {
    std::vector<void*> v;
    hipStream_t s;
    ~Blocks() {
        (void)hipStreamSynchronize(s);
        for (void* p : v) mcg_dev_free(p);
    }
    int upload(const void* src, size_t bytes, void** out) {
        if (int e = mcg_dev_alloc(bytes, out)) return e;
        v.push_back(*out);
        MCG_HIP(hipMemcpyAsync(*out, src, bytes, hipMemcpyHostToDevice, s));
        return MCG_OK;
    }
};

// every slot the kernels will read names a row of its buffer
int check_slots(const int32_t* dev, int entries, int per_entry, int rows, const char* what, hipStream_t s) {
    std::vector<int32_t> t((size_t)entries * 4);
    MCG_HIP(hipMemcpyAsync(t.data(), dev, t.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MCG_HIP(hipStreamSynchronize(s));
    for (int e = 0; e < entries; ++e)
        for (int q = 0; q < per_entry; ++q)
            if (t[(size_t)e * 4 + q] < 0 || t[(size_t)e * 4 + q] >= rows) {
                mcg_set_error("mcg_debug_gemm: %s[%d][%d] = %d names no row of its %d-row buffer", what, e, q, t[(size_t)e * 4 + q], rows);
                return MCG_ERR_ARG;
            }
    return MCG_OK;
}

}  // namespace

extern "C" int mcg_debug_gemm_pack(const float* w_host, int n_out, int K1, int K2, int kind, void* dst_host, int64_t dst_capacity,
                                   int64_t* n_elems_host) {
    if (!w_host || !n_elems_host || n_out < 1 || n_out > (1 << 16) || K1 < 4 || K1 % 4 != 0 || K2 < 0 || K2 % 4 != 0 || K1 > (1 << 16) ||
        K2 > (1 << 16) || kind < MCG_GEMM_PACK4 || kind > MCG_GEMM_PACK16X3) {
        mcg_set_error("mcg_debug_gemm_pack: needs w_host, n_elems_host, n_out in 1 .. 2^16, K1 % 4 == 0 in 4 .. 2^16, K2 % 4 == 0 in 0 .. 2^16, kind 0 .. 2");
        return MCG_ERR_ARG;
    }
    std::vector<float> f;
    std::vector<uint16_t> h;
    pack_segments(kind, w_host, n_out, K1, K2, f, h);
    const int64_t n = kind == MCG_GEMM_PACK4 ? (int64_t)f.size() : (int64_t)h.size();
    *n_elems_host = n;
    if (!dst_host) return MCG_OK;
    if (dst_capacity < n) {
        mcg_set_error("mcg_debug_gemm_pack: the pack has %lld elements, dst_host holds %lld", (long long)n, (long long)dst_capacity);
        return MCG_ERR_ARG;
    }
    if (kind == MCG_GEMM_PACK4) __builtin_memcpy(dst_host, f.data(), f.size() * sizeof(float));
    else __builtin_memcpy(dst_host, h.data(), h.size() * sizeof(uint16_t));
    return MCG_OK;
}

extern "C" int mcg_debug_gemm(const mcg_gemm_desc* dp, mcg_gemm_ran* ran_host, void* stream) {
    if (!check_desc(dp, ran_host)) return MCG_ERR_ARG;
    const mcg_gemm_desc& d = *dp;
    hipStream_t s = (hipStream_t)stream;
    const int n_tiles = n_tiles_of(d.n_out);
    if (d.a2_rows)
        if (int e = check_slots(d.a2_rows, d.M, gather_width(d), d.a2_src_rows, "a2_rows", s)) return e;
    if (d.side_x)
        if (int e = check_slots(d.side_slots, d.side_M, 4, d.side_u_rows, "side_slots", s)) return e;

    std::vector<float> f;
    std::vector<uint16_t> h;
    const int kind = d.family == MCG_GEMM_BF16 ? MCG_GEMM_PACK16 : d.family == MCG_GEMM_X6 ? MCG_GEMM_PACK16X3 : MCG_GEMM_PACK4;
    pack_segments(kind, d.w_host, d.n_out, d.K1, d.K2, f, h);
    Blocks blocks{{}, s};
    McgGemmArgs a{};
    void* bp = nullptr;
    if (int e = kind == MCG_GEMM_PACK4 ? blocks.upload(f.data(), f.size() * sizeof(float), &bp)
                                       : blocks.upload(h.data(), h.size() * sizeof(uint16_t), &bp)) return e;
    a.Bp = static_cast<const float*>(bp);
    if (d.bias) {
        void* b = nullptr;
        if (int e = mcg_dev_alloc((size_t)16 * n_tiles * sizeof(float), &b)) return e;
        blocks.v.push_back(b);
        MCG_HIP(hipMemsetAsync(b, 0, (size_t)16 * n_tiles * sizeof(float), s));
        MCG_HIP(hipMemcpyAsync(b, d.bias, (size_t)d.n_out * sizeof(float), hipMemcpyDeviceToDevice, s));
        a.bias = static_cast<const float*>(b);
    }
    a.A1 = d.A1; a.lda1 = d.lda1; a.K1 = d.K1;
    a.A2 = d.A2; a.lda2 = d.lda2; a.K2 = d.K2;
    a.resid = d.resid; a.ldr = d.ldr; a.C = d.C; a.ldc = d.ldc;
    a.M = d.M; a.n_tiles = n_tiles; a.n_store = d.n_store; a.act = d.act;
    a.a2_rows = reinterpret_cast<const int4*>(d.a2_rows); a.a2_nsum = d.a2_nsum;
    a.side_u = d.side_u; a.side_slots = reinterpret_cast<const int4*>(d.side_slots); a.side_x = d.side_x; a.side_M = d.side_M;
    a.c_blocked = d.c_blocked;
    switch (d.family) {
        case MCG_GEMM_F32: MCG_HIP(mcg_gemm_launch(a, d.rn, s)); break;
        case MCG_GEMM_F32ROWS16: MCG_HIP(mcg_gemm16_launch(a, d.rn, d.mr, d.deep != 0, s)); break;
        case MCG_GEMM_BF16: MCG_HIP(mcg_gemm_bf16_launch(a, d.rn, d.lds, s)); break;
        default: MCG_HIP(mcg_gemm_x6_launch(a, d.rn, s)); break;
    }
    const McgGemmRan& r = mcg_gemm_last_launch();
    *ran_host = mcg_gemm_ran{r.kernel, r.rn, r.mr, r.ring, r.gather, r.resid, r.seg2, 0};
    MCG_HIP(hipStreamSynchronize(s));
    return MCG_OK;
}
