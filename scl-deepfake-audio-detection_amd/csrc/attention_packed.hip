// attention_packed.hip — a variable-length batch with its valid frames packed back to back: rows 0 .. Mv-1 of qkv / ctx / dctx / dqkv hold
// the frames of all utterances one after the other, and nothing else is computed by the row-wise kernels around the attention (LayerNorm,
// the four linears and their gradients).  Only the attention has to know where an utterance starts and ends:
//   row0[B + 1]  int32 on the device: row0[0] = 0, row0[b + 1] = row0[b] + frames[b], row0[B] = Mv.  Utterance b owns packed rows
//                row0[b] .. row0[b + 1] - 1; its length Tb = row0[b + 1] - row0[b] is clamped to [1, T] and to the launch's Mq rows on
//                the device for memory safety, and scl_packed_check_rows validates the host copy before the upload.
//   Mq           the launch's row count (Mv <= Mq): rows [Mv, Mq) belong to no utterance.  Mv is READ FROM row0[B] on the device, so a
//                recorded launch stays valid when the lengths change within the same Mq.
//
//   scl_attn_fwd_packed / _drop   the streaming forward of attn_stream_body.h with Rows::Packed: the body of attention_varlen.hip with the
//                                 utterance's rows addressed from row0[b] instead of b*T.  lse and the dropout mask index stay in the padded
//                                 (b, h, q, T) space: rows row0[b] + t of ctx carry the bits scl_attn_fwd_varlen(_drop) gives at b*T + t.
//   scl_attn_bwd_packed           the deterministic streaming backward likewise (delta workspace in the padded space).
//                                 THE STORES: where the padded kernels zero-fill rows >= klen[b], the packed rows behind an utterance
//                                 belong to the next one.  Nothing is stored at or beyond Tb, and a 64-query / 128-key block that starts
//                                 there returns before its first barrier without a store.  Rows [Mv, Mq) are written as zeros (ctx by the
//                                 forward, dqkv by the backward): the gradients of rows that belong to nobody are exactly 0.
// Head dim 64 is compiled here; the entries hand head dims 72..128 to attention_wide.hip (the same bodies with a padded head dim).
//   scl_pack_rows                 dst[row0[b] + t] = src[b*T + t] for t < Tb; dst rows [Mv, Mq) = 0 (padded source rows are not read).
//   scl_unpack_rows               dst[b*T + t] = t < Tb ? src[row0[b] + t] : 0.  Either way every row of the destination is written.
#include "attn_stream_body.h"
#include "attn_wide.h"      // head dims 72..128: attention_wide.hip

namespace {

template <bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_packed_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, float* __restrict__ lse,
                                                              const int* __restrict__ row0, int T, int H, int nqb, int B, int Mq, float scale,
                                                              float drop_p, uint32_t drop_seed) {
    attn_stream_fwd_body<DROP, Rows::Packed>(qkv, ctx, lse, row0, T, H, nqb, B, Mq, scale, drop_p, drop_seed);
}

__global__ __launch_bounds__(256) void attn_delta_packed_kernel(const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx,
                                                                float* __restrict__ delta, const int* __restrict__ row0, int64_t rows, int T, int H,
                                                                int Mq) {
    attn_stream_delta_body<Rows::Packed>(ctx, dctx, delta, row0, rows, T, H, Mq);
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_packed_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   bf16_t* __restrict__ dqkv, const int* __restrict__ row0, int T, int H, int nkw,
                                                                   int Mq, float scale, float drop_p, uint32_t drop_seed) {
    attn_stream_dkdv_body<DROP, Rows::Packed>(qkv, dctx, lse, delta, dqkv, row0, T, H, nkw, Mq, scale, drop_p, drop_seed);
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_packed_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16_t* __restrict__ dqkv, const int* __restrict__ row0, int T, int H, int nqb,
                                                                 int B, int Mq, float scale, float drop_p, uint32_t drop_seed) {
    attn_stream_dq_body<DROP, Rows::Packed>(qkv, dctx, lse, delta, dqkv, row0, T, H, nqb, B, Mq, scale, drop_p, drop_seed);
}

// ---- pack / unpack: one thread per 16 bytes, rows of vec_per_row vectors; both walk the PADDED (b, t) space ---------------------------------
__global__ __launch_bounds__(256) void pack_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* __restrict__ row0, int B,
                                                        int T, int vec_per_row, int Mq) {
    const int64_t per_utt = (int64_t)T * vec_per_row, n = (int64_t)B * per_utt;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / per_utt);
        const int64_t in_utt = i - (int64_t)b * per_utt;
        const int t = (int)(in_utt / vec_per_row);
        const UttRows<Rows::Packed> utt(row0, b, T, Mq);
        if (t < utt.Tb) dst[utt.r0 * vec_per_row + in_utt] = src[i];
    }
    zero_tail_vectors(dst, row0, B, Mq, vec_per_row);
}

__global__ __launch_bounds__(256) void unpack_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* __restrict__ row0, int B,
                                                          int T, int vec_per_row, int Mq) {
    const int64_t per_utt = (int64_t)T * vec_per_row, n = (int64_t)B * per_utt;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / per_utt);
        const int64_t in_utt = i - (int64_t)b * per_utt;
        const int t = (int)(in_utt / vec_per_row);
        const UttRows<Rows::Packed> utt(row0, b, T, Mq);
        dst[i] = t < utt.Tb ? src[utt.r0 * vec_per_row + in_utt] : make_uint4(0u, 0u, 0u, 0u);
    }
}

unsigned rows_grid(int64_t n) { const int64_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

}  // namespace

extern "C" int scl_packed_check_rows(const int32_t* row0_host, int B, int T, int Mq) {
    SCL_REQUIRE(row0_host && B > 0 && T >= 1 && Mq >= B, "packed_check_rows: bad args");
    SCL_REQUIRE(row0_host[0] == 0, "packed: row0[0] is %d, not 0", row0_host[0]);
    for (int b = 0; b < B; ++b) {
        const int64_t n = (int64_t)row0_host[b + 1] - row0_host[b];
        SCL_REQUIRE(n >= 1 && n <= T, "packed: utterance %d holds %lld rows (row0 %d .. %d), outside 1..%d frames", b, (long long)n, row0_host[b],
                    row0_host[b + 1], T);
    }
    SCL_REQUIRE(row0_host[B] <= Mq, "packed: %d valid rows do not fit the launch's %d rows", row0_host[B], Mq);
    return 0;
}

// WIDE: the call that hands head dims 72..128 to attention_wide.hip (which checks Mq and the grid itself)
#define PACKED_ATTN_ARGS(name, WIDE)                                                                                        \
    if (scl_attn_wide_takes(D)) return WIDE;                                                                                \
    SCL_REQUIRE(D == LD, name ": " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);                                                    \
    SCL_REQUIRE(Mq >= B && (int64_t)Mq <= ((int64_t)B * T + 63) / 64 * 64, name ": need B <= Mq <= roundup(B * T, 64)");     \
    const int nqb = (T + LQB - 1) / LQB;                                                                                    \
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, name ": grid too large")

extern "C" int scl_attn_fwd_packed(const void* qkv, void* ctx, float* lse, const int32_t* row0, int B, int T, int H, int D, int Mq, float scale,
                                   void* stream) {
    SCL_REQUIRE(qkv && ctx && lse && row0 && B > 0 && H > 0 && T >= 1, "attn_fwd_packed: bad args");
    PACKED_ATTN_ARGS("attn_fwd_packed", scl_attn_wide_fwd(SCL_ROWS_PACKED, "scl_attn_fwd_packed", qkv, ctx, lse, row0, B, T, H, D, Mq, scale, 0.f, 0u, stream));
    hipLaunchKernelGGL(attn_fwd_packed_kernel<false>, dim3((unsigned)(B * H * nqb)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv,
                       (bf16_t*)ctx, lse, (const int*)row0, T, H, nqb, B, Mq, scale, 0.f, 0u);
    return scl_check_launch("scl_attn_fwd_packed");
}

extern "C" int scl_attn_fwd_packed_drop(const void* qkv, void* ctx, float* lse, const int32_t* row0, int B, int T, int H, int D, int Mq, float scale,
                                        float drop_p, uint32_t drop_seed, void* stream) {
    SCL_REQUIRE(qkv && ctx && lse && row0 && B > 0 && H > 0 && T >= 1 && drop_p >= 0.f && drop_p < 1.f, "attn_fwd_packed_drop: bad args");
    PACKED_ATTN_ARGS("attn_fwd_packed_drop",
                     scl_attn_wide_fwd(SCL_ROWS_PACKED, "scl_attn_fwd_packed_drop", qkv, ctx, lse, row0, B, T, H, D, Mq, scale, drop_p, drop_seed, stream));
    const dim3 grid((unsigned)(B * H * nqb));
    if (drop_p > 0.f)
        hipLaunchKernelGGL(attn_fwd_packed_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)ctx, lse,
                           (const int*)row0, T, H, nqb, B, Mq, scale, drop_p, drop_seed);
    else
        hipLaunchKernelGGL(attn_fwd_packed_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)ctx, lse,
                           (const int*)row0, T, H, nqb, B, Mq, scale, drop_p, drop_seed);
    return scl_check_launch("scl_attn_fwd_packed_drop");
}

// workspace: scl_attn_long_ws_bytes(B, T, H) bytes (delta, f32 [B, H, T]: the padded space)
extern "C" int scl_attn_bwd_packed(const void* qkv, const void* ctx, const void* dctx, const float* lse, const int32_t* row0, void* dqkv, void* ws,
                                   int B, int T, int H, int D, int Mq, float scale, float drop_p, uint32_t drop_seed, void* stream) {
    SCL_REQUIRE(qkv && ctx && dctx && lse && row0 && dqkv && ws && B > 0 && H > 0 && T >= 1 && drop_p >= 0.f && drop_p < 1.f,
                "attn_bwd_packed: bad args");
    PACKED_ATTN_ARGS("attn_bwd_packed", scl_attn_wide_bwd(SCL_ROWS_PACKED, "scl_attn_bwd_packed", qkv, ctx, dctx, lse, row0, dqkv, ws, B, T, H, D, Mq,
                                                          scale, drop_p, drop_seed, stream));
    const int nkw = (T + LKW - 1) / LKW;
    hipStream_t s = (hipStream_t)stream;
    float* delta = (float*)ws;
    const int64_t rows = (int64_t)B * T * H;
    hipLaunchKernelGGL(attn_delta_packed_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, s, (const bf16_t*)ctx, (const bf16_t*)dctx,
                       delta, (const int*)row0, rows, T, H, Mq);
    int rc = scl_check_launch("scl_attn_bwd_packed (delta)");
    if (rc) return rc;
#define ATT_BWD_PACKED(DR)                                                                                                                        \
    hipLaunchKernelGGL(attn_bwd_dkdv_packed_kernel<DR>, dim3((unsigned)(B * H * nkw)), dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dctx, \
                       lse, (const float*)delta, (bf16_t*)dqkv, (const int*)row0, T, H, nkw, Mq, scale, drop_p, drop_seed);                      \
    hipLaunchKernelGGL(attn_bwd_dq_packed_kernel<DR>, dim3((unsigned)(B * H * nqb)), dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dctx,   \
                       lse, (const float*)delta, (bf16_t*)dqkv, (const int*)row0, T, H, nqb, B, Mq, scale, drop_p, drop_seed)
    if (drop_p > 0.f) { ATT_BWD_PACKED(true); }
    else { ATT_BWD_PACKED(false); }
#undef ATT_BWD_PACKED
    return scl_check_launch("scl_attn_bwd_packed");
}
#undef PACKED_ATTN_ARGS

#define PACK_ROWS_ARGS(name)                                                                                                         \
    SCL_REQUIRE(src && dst && row0 && B > 0 && T > 0 && C > 0 && (C & 7) == 0, name ": need C %% 8 == 0");                             \
    SCL_REQUIRE(Mq >= B && (int64_t)Mq <= ((int64_t)B * T + 63) / 64 * 64, name ": need B <= Mq <= roundup(B * T, 64)");               \
    const int vec_per_row = is_f32 ? C / 4 : C / 8;                                                                                  \
    const unsigned grid = rows_grid((int64_t)B * T * vec_per_row)

extern "C" int scl_pack_rows(const void* src, void* dst, int is_f32, const int32_t* row0, int B, int T, int C, int Mq, void* stream) {
    PACK_ROWS_ARGS("pack_rows");
    hipLaunchKernelGGL(pack_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, (uint4*)dst, (const int*)row0, B, T,
                       vec_per_row, Mq);
    return scl_check_launch("scl_pack_rows");
}

extern "C" int scl_unpack_rows(const void* src, void* dst, int is_f32, const int32_t* row0, int B, int T, int C, int Mq, void* stream) {
    PACK_ROWS_ARGS("unpack_rows");
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, (uint4*)dst, (const int*)row0, B, T,
                       vec_per_row, Mq);
    return scl_check_launch("scl_unpack_rows");
}
#undef PACK_ROWS_ARGS
