// attention_wide.hip — the streaming attention for head dims 72..128 (D % 8 == 0): the bodies of attn_wide_body.h with a padded head dim
// DP = 96 (D = 72..96) or DP = 128 (D = 104..128), in all three row layouts (Rows::Fixed / Padded / Packed), forward and backward, with
// and without attention dropout.  The tile scheme, the layouts, lse, the delta workspace and the dropout mask index are those of the 64
// family (attention_long.hip, attention_varlen.hip, attention_packed.hip), whose C ABI entries dispatch here on D.
//
// The padding exists in registers and LDS only.  In memory a head is D columns wide; columns D..DP-1 of a head's row are the next head's
// data (or the next section's, or lie past the buffer) and are never read or written: a 16-byte chunk c is loaded when 8 c < D and is
// zero otherwise, zero columns add 0 to Q K^T and dO V^T, 4-column output groups at or beyond D are not stored, and the last 16-column
// tile gets no MFMA when it lies at or beyond D.
//
// LDS per workgroup: forward 2 x 2 x 64 x 2 DP B = 48 / 64 KiB, dQ 2 x 3 x 64 x 2 DP B = 72 / 96 KiB, dK / dV 2 x (4 x 32 x 2 DP + 256) B =
// 48.5 / 64.5 KiB.  The fixed layout's dK / dV is the shared body too (the hand-written one of attention_long.hip is for head dim 64).
#include "attn_wide_body.h"
#include "attn_wide.h"

namespace {

template <bool DROP, Rows L, int DP>
__global__ __launch_bounds__(256) void attn_fwd_wide_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, float* __restrict__ lse,
                                                            const int* __restrict__ lens, int T, int H, int D, int nqb, int B, int Mq, float scale,
                                                            float drop_p, uint32_t drop_seed) {
    wide::attn_stream_fwd_body<DROP, L, DP>(qkv, ctx, lse, lens, T, H, nqb, B, Mq, scale, drop_p, drop_seed, D);
}

template <Rows L>
__global__ __launch_bounds__(256) void attn_delta_wide_kernel(const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx,
                                                              float* __restrict__ delta, const int* __restrict__ lens, int64_t rows, int T, int H,
                                                              int D, int Mq) {
    wide::attn_stream_delta_body<L>(ctx, dctx, delta, lens, rows, T, H, Mq, D);
}

template <bool DROP, Rows L, int DP>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_wide_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16_t* __restrict__ dqkv, const int* __restrict__ lens, int T, int H, int D, int nkw,
                                                                 int Mq, float scale, float drop_p, uint32_t drop_seed) {
    wide::attn_stream_dkdv_body<DROP, L, DP>(qkv, dctx, lse, delta, dqkv, lens, T, H, nkw, Mq, scale, drop_p, drop_seed, D);
}

template <bool DROP, Rows L, int DP>
__global__ __launch_bounds__(256) void attn_bwd_dq_wide_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               bf16_t* __restrict__ dqkv, const int* __restrict__ lens, int T, int H, int D, int nqb,
                                                               int B, int Mq, float scale, float drop_p, uint32_t drop_seed) {
    wide::attn_stream_dq_body<DROP, L, DP>(qkv, dctx, lse, delta, dqkv, lens, T, H, nqb, B, Mq, scale, drop_p, drop_seed, D);
}

struct WideArgs {
    const bf16_t *qkv, *ctx_in, *dctx;
    bf16_t *ctx, *dqkv;
    float* lse;
    const float* lse_in;
    float* delta;
    const int* lens;
    int B, T, H, D, Mq;
    float scale, drop_p;
    uint32_t drop_seed;
    hipStream_t s;
};

// the launches, as operations that by_rows_and_width instantiates per (layout, padded head dim)
template <bool DROP>
struct LaunchFwd {
    template <Rows L, int DP>
    static void run(const WideArgs& a) {
        const int nqb = (a.T + LQB - 1) / LQB;
        hipLaunchKernelGGL((attn_fwd_wide_kernel<DROP, L, DP>), dim3((unsigned)(a.B * a.H * nqb)), dim3(256), 0, a.s, a.qkv, a.ctx, a.lse, a.lens,
                           a.T, a.H, a.D, nqb, a.B, a.Mq, a.scale, a.drop_p, a.drop_seed);
    }
};

struct LaunchDelta {
    template <Rows L, int>      // one kernel per layout: the pieces of a row are counted from D
    static void run(const WideArgs& a) {
        const int64_t rows = (int64_t)a.B * a.T * a.H;
        hipLaunchKernelGGL(attn_delta_wide_kernel<L>, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, a.s, a.ctx_in, a.dctx, a.delta,
                           a.lens, rows, a.T, a.H, a.D, a.Mq);
    }
};

template <bool DROP>
struct LaunchBwd {
    template <Rows L, int DP>
    static void run(const WideArgs& a) {
        const int nqb = (a.T + LQB - 1) / LQB, nkw = (a.T + LKW - 1) / LKW;
        hipLaunchKernelGGL((attn_bwd_dkdv_wide_kernel<DROP, L, DP>), dim3((unsigned)(a.B * a.H * nkw)), dim3(256), 0, a.s, a.qkv, a.dctx, a.lse_in,
                           (const float*)a.delta, a.dqkv, a.lens, a.T, a.H, a.D, nkw, a.Mq, a.scale, a.drop_p, a.drop_seed);
        hipLaunchKernelGGL((attn_bwd_dq_wide_kernel<DROP, L, DP>), dim3((unsigned)(a.B * a.H * nqb)), dim3(256), 0, a.s, a.qkv, a.dctx, a.lse_in,
                           (const float*)a.delta, a.dqkv, a.lens, a.T, a.H, a.D, nqb, a.B, a.Mq, a.scale, a.drop_p, a.drop_seed);
    }
};

template <typename Op, Rows L>
void by_width(const WideArgs& a) {
    if (a.D <= 96) Op::template run<L, 96>(a);
    else Op::template run<L, 128>(a);
}
template <typename Op>
void by_rows_and_width(SclAttnRows rows, const WideArgs& a) {
    if (rows == SCL_ROWS_FIXED) by_width<Op, Rows::Fixed>(a);
    else if (rows == SCL_ROWS_PADDED) by_width<Op, Rows::Padded>(a);
    else by_width<Op, Rows::Packed>(a);
}

int check(SclAttnRows rows, const char* who, const void* lens, int B, int T, int H, int D, int Mq) {
    SCL_REQUIRE(scl_attn_wide_takes(D), "%s: " SCL_ATTN_HEAD_DIMS " (got D=%d)", who, D);
    SCL_REQUIRE(B > 0 && H > 0 && T >= 1 && (rows == SCL_ROWS_FIXED) == (lens == nullptr), "%s: bad args", who);
    SCL_REQUIRE(rows != SCL_ROWS_PACKED || (Mq >= B && (int64_t)Mq <= ((int64_t)B * T + 63) / 64 * 64), "%s: need B <= Mq <= roundup(B * T, 64)", who);
    SCL_REQUIRE((int64_t)B * H * ((T + LQB - 1) / LQB) < 0x7FFFFFFF, "%s: grid too large", who);
    return 0;
}

}  // namespace

int scl_attn_wide_fwd(SclAttnRows rows, const char* who, const void* qkv, void* ctx, float* lse, const int32_t* lens, int B, int T, int H, int D,
                      int Mq, float scale, float drop_p, uint32_t drop_seed, void* stream) {
    if (int rc = check(rows, who, lens, B, T, H, D, Mq)) return rc;
    SCL_REQUIRE(qkv && ctx && lse && drop_p >= 0.f && drop_p < 1.f, "%s: bad args", who);
    WideArgs a{};
    a.qkv = (const bf16_t*)qkv; a.ctx = (bf16_t*)ctx; a.lse = lse; a.lens = (const int*)lens;
    a.B = B; a.T = T; a.H = H; a.D = D; a.Mq = Mq; a.scale = scale; a.drop_p = drop_p; a.drop_seed = drop_seed; a.s = (hipStream_t)stream;
    if (drop_p > 0.f) by_rows_and_width<LaunchFwd<true>>(rows, a);
    else by_rows_and_width<LaunchFwd<false>>(rows, a);
    return scl_check_launch(who);
}

int scl_attn_wide_bwd(SclAttnRows rows, const char* who, const void* qkv, const void* ctx, const void* dctx, const float* lse, const int32_t* lens,
                      void* dqkv, void* ws, int B, int T, int H, int D, int Mq, float scale, float drop_p, uint32_t drop_seed, void* stream) {
    if (int rc = check(rows, who, lens, B, T, H, D, Mq)) return rc;
    SCL_REQUIRE(qkv && ctx && dctx && lse && dqkv && ws && drop_p >= 0.f && drop_p < 1.f, "%s: bad args", who);
    WideArgs a{};
    a.qkv = (const bf16_t*)qkv; a.ctx_in = (const bf16_t*)ctx; a.dctx = (const bf16_t*)dctx; a.lse_in = lse; a.dqkv = (bf16_t*)dqkv;
    a.delta = (float*)ws; a.lens = (const int*)lens;
    a.B = B; a.T = T; a.H = H; a.D = D; a.Mq = Mq; a.scale = scale; a.drop_p = drop_p; a.drop_seed = drop_seed; a.s = (hipStream_t)stream;
    by_rows_and_width<LaunchDelta>(rows, a);
    if (int rc = scl_check_launch(who)) return rc;
    if (drop_p > 0.f) by_rows_and_width<LaunchBwd<true>>(rows, a);
    else by_rows_and_width<LaunchBwd<false>>(rows, a);
    return scl_check_launch(who);
}
