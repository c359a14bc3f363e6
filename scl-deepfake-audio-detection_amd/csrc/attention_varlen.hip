// attention_varlen.hip — a zero-padded batch of utterances of different lengths: per-utterance frame counts klen[b] (int32 on the
// device, 1 <= klen[b] <= T) play the part of fairseq's padding_mask, for scoring and for training.
//
//   scl_attn_fwd_varlen          the streaming forward (attn_stream_body.h) with the key loop, the K / V staging and the last block's
//                                mask running to klen[b] instead of T: keys >= klen[b] are never loaded, and a block of 64 queries that
//                                starts at or beyond klen[b] writes zeros and leaves before the first barrier.  klen[b] is one value per
//                                workgroup, so the trip count and the early exit are workgroup-uniform.  Per query the blocks are visited
//                                in the order of scl_attn_fwd_long at T = klen[b]: rows < klen[b] carry the same bits.
//   scl_attn_fwd_varlen_drop     the same with attention dropout: keep-mask hash(seed, ((b*H + h)*T + q)*T + k) with the PADDED T, the
//                                index of the fixed-length kernels.
//   scl_attn_bwd_varlen          the deterministic streaming backward of attn_stream_body.h (delta, dK / dV per 128 keys, dQ per 64
//                                queries, no atomics) with query tiles and key blocks running to klen[b].  A dK / dV or dQ block that
//                                starts at or beyond klen[b] writes zeros into its rows of dqkv and leaves before its first barrier;
//                                rows >= klen[b] of the last partial block are stored as zeros: EVERY row of dqkv is written, rows
//                                >= klen[b] are exactly 0 and are never loaded (they may hold NaN).  Without dropout, rows < klen[b]
//                                carry the bits of scl_attn_bwd_long on the utterance alone at T = klen[b].
//   scl_softmax_fwd_f32_varlen   the fp32 row soft-max of the fp32 scoring path over the first klen[row / rows_per_utt] columns (row in
//                                registers up to 512 columns, looped above); every other column up to Tp is written as 0.
//   scl_zero_tail_rows           x[b][t >= len[b]][:] = 0 (fairseq's index_put(x, padding_mask, 0) after post_extract_proj; feats tail).
//   scl_meanpool_fwd_varlen      emb[b] = sum_{t < len[b]} h[b][t] / len[b], the summation order of scl_meanpool_fwd.
//   scl_meanpool_bwd_varlen      scl_meanpool_bwd (activation derivative and head-dropout mask fused) scaled by 1 / len[b]; rows
//                                t >= len[b] are written as 0.
// The device-side counts are clamped to [1, T] for memory safety; scl_varlen_check_lengths validates the host copy before the upload.
// The attention kernels are the bodies of attn_stream_body.h in the padded layout (Rows::Padded), compiled here for head dim 64; the
// entries hand head dims 72..128 to attention_wide.hip.  attention_long.hip holds the same bodies
// for batches without a length array (Rows::Fixed) and attention_packed.hip for frames packed back to back (Rows::Packed).
#include "attn_stream_body.h"
#include "attn_wide.h"      // head dims 72..128: attention_wide.hip

namespace {

// the padded layout's kernels: the shared bodies with Rows::Padded (utterance b at rows b*T, every row of the outputs written)
template <bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_varlen_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, float* __restrict__ lse,
                                                              const int* __restrict__ klen, int T, int H, int nqb, float scale,
                                                              float drop_p, uint32_t drop_seed) {
    attn_stream_fwd_body<DROP, Rows::Padded>(qkv, ctx, lse, klen, T, H, nqb, 0, 0, scale, drop_p, drop_seed);
}

__global__ __launch_bounds__(256) void attn_delta_varlen_kernel(const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx,
                                                                float* __restrict__ delta, const int* __restrict__ klen, int64_t rows, int T, int H) {
    attn_stream_delta_body<Rows::Padded>(ctx, dctx, delta, klen, rows, T, H, 0);
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_varlen_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   bf16_t* __restrict__ dqkv, const int* __restrict__ klen, int T, int H, int nkw,
                                                                   float scale, float drop_p, uint32_t drop_seed) {
    attn_stream_dkdv_body<DROP, Rows::Padded>(qkv, dctx, lse, delta, dqkv, klen, T, H, nkw, 0, scale, drop_p, drop_seed);
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_varlen_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16_t* __restrict__ dqkv, const int* __restrict__ klen, int T, int H, int nqb,
                                                                 float scale, float drop_p, uint32_t drop_seed) {
    attn_stream_dq_body<DROP, Rows::Padded>(qkv, dctx, lse, delta, dqkv, klen, T, H, nqb, 0, 0, scale, drop_p, drop_seed);
}

// ---- fp32 row soft-max over the first klen columns ----------------------------------------------------------------------------------
constexpr int MAXV = 8;      // up to 512 columns kept in registers (attention.hip's softmax_fwd_kernel<float>)

template <bool LOOPED>
__global__ __launch_bounds__(256) void softmax_fwd_f32_varlen_kernel(const float* __restrict__ S, float* __restrict__ P, const int* __restrict__ klen,
                                                                     int64_t R, int rows_per_utt, int T, int ldS, int Tp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int Tv = clamp_len(klen[row / rows_per_utt], T);
    const float* s = S + row * ldS;
    float* p = P + row * Tp;
    if constexpr (!LOOPED) {
        float v[MAXV];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = i * 64 + lane;
            v[i] = c < Tv ? s[c] : -INFINITY;
            mx = fmaxf(mx, v[i]);
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = i * 64 + lane;
            v[i] = c < Tv ? __expf(v[i] - mx) : 0.f;
            sum += v[i];
        }
        const float inv = 1.0f / wave_sum(sum);
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = i * 64 + lane;
            if (c < Tp) p[c] = v[i] * inv;
        }
    } else {      // online (max, sum) pass, then the write pass
        softmax_f32_looped_row(s, p, Tv, Tp, lane);
    }
}

// ---- zero the padded rows: one thread per 16 bytes, rows of C * sizeof(TA) bytes (a multiple of 16) -------------------------------------
__global__ __launch_bounds__(256) void zero_tail_rows_kernel(uint4* __restrict__ x, const int* __restrict__ len, int B, int T, int vec_per_row) {
    const int64_t per_utt = (int64_t)T * vec_per_row, n = (int64_t)B * per_utt;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / per_utt);
        const int t = (int)((i - (int64_t)b * per_utt) / vec_per_row);
        if (t >= clamp_len(len[b], T)) x[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- emb[b][c] = sum_{t < len[b]} h[b][t][c] / len[b]: elementwise.hip's meanpool_fwd_kernel (4 frame groups x 128 channel lanes, the
// four partial sums combined in a fixed order) over the utterance's own frames
__device__ __forceinline__ float ld_act(const bf16_t* p, int64_t i) { return bf2f(p[i]); }
__device__ __forceinline__ float ld_act(const float* p, int64_t i) { return p[i]; }
template <typename TA>
__global__ __launch_bounds__(512) void meanpool_fwd_varlen_kernel(const TA* __restrict__ h, float* __restrict__ emb, const int* __restrict__ len,
                                                                  int T, int C) {
    __shared__ float red[4][128];
    const int b = blockIdx.x, g = threadIdx.x >> 7, l = threadIdx.x & 127;
    const int Tb = clamp_len(len[b], T);
    for (int c0 = 0; c0 < C; c0 += 128) {
        const int c = c0 + l;
        float s = 0.f;
        if (c < C)
            for (int t = g; t < Tb; t += 4) s += ld_act(h, ((int64_t)b * T + t) * C + c);
        red[g][l] = s;
        __syncthreads();
        if (g == 0 && c < C) emb[(int64_t)b * C + c] = (((red[0][l] + red[1][l]) + red[2][l]) + red[3][l]) / (float)Tb;
        __syncthreads();
    }
}

// d_pre[b][t][c] = d_emb[b][c] / len[b] * dropmask(seed, idx) * act'(pre[b][t][c]) for t < len[b], 0 beyond: elementwise.hip's meanpool_bwd_kernel
// (the same element index feeds the mask) over the utterance's own frames; pre rows beyond them are not read
__device__ __forceinline__ void st_act(bf16_t* p, int64_t i, float v) { p[i] = f2bf(v); }
__device__ __forceinline__ void st_act(float* p, int64_t i, float v) { p[i] = v; }
template <typename TA>
__global__ void meanpool_bwd_varlen_kernel(const float* __restrict__ demb, const TA* __restrict__ pre, TA* __restrict__ dpre,
                                           const int* __restrict__ len, int B, int T, int C, int ract, float drop_p, uint32_t seed) {
    const int64_t n = (int64_t)B * T * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int b = (int)(i / ((int64_t)T * C));
        const int t = (int)((i / C) % T);
        const int Tb = clamp_len(len[b], T);
        float v = 0.f;
        if (t < Tb) {
            v = demb[(int64_t)b * C + c] / (float)Tb;
            if (drop_p > 0.f) v *= dropout_scale(seed, (uint64_t)i, drop_p);
            v *= act_grad_f(ract, ld_act(pre, i));
        }
        st_act(dpre, i, v);
    }
}

}  // namespace

extern "C" int scl_varlen_check_lengths(const int32_t* len_host, int B, int T) {
    SCL_REQUIRE(len_host && B > 0 && T >= 1, "varlen_check_lengths: bad args");
    for (int b = 0; b < B; ++b)
        SCL_REQUIRE(len_host[b] >= 1 && len_host[b] <= T, "varlen: length %d of utterance %d is outside 1..%d frames", len_host[b], b, T);
    return 0;
}

extern "C" int scl_attn_fwd_varlen(const void* qkv, void* ctx, float* lse, const int32_t* klen, int B, int T, int H, int D, float scale,
                                   void* stream) {
    SCL_REQUIRE(qkv && ctx && lse && klen && B > 0 && H > 0 && T >= 1, "attn_fwd_varlen: bad args");
    if (scl_attn_wide_takes(D))
        return scl_attn_wide_fwd(SCL_ROWS_PADDED, "scl_attn_fwd_varlen", qkv, ctx, lse, klen, B, T, H, D, 0, scale, 0.f, 0u, stream);
    SCL_REQUIRE(D == LD, "attn_fwd_varlen: " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);
    const int nqb = (T + LQB - 1) / LQB;
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, "attn_fwd_varlen: grid too large");
    hipLaunchKernelGGL(attn_fwd_varlen_kernel<false>, dim3((unsigned)(B * H * nqb)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv,
                       (bf16_t*)ctx, lse, (const int*)klen, T, H, nqb, scale, 0.f, 0u);
    return scl_check_launch("scl_attn_fwd_varlen");
}

extern "C" int scl_attn_fwd_varlen_drop(const void* qkv, void* ctx, float* lse, const int32_t* klen, int B, int T, int H, int D, float scale,
                                        float drop_p, uint32_t drop_seed, void* stream) {
    SCL_REQUIRE(qkv && ctx && lse && klen && B > 0 && H > 0 && T >= 1 && drop_p >= 0.f && drop_p < 1.f, "attn_fwd_varlen_drop: bad args");
    if (scl_attn_wide_takes(D))
        return scl_attn_wide_fwd(SCL_ROWS_PADDED, "scl_attn_fwd_varlen_drop", qkv, ctx, lse, klen, B, T, H, D, 0, scale, drop_p, drop_seed, stream);
    SCL_REQUIRE(D == LD, "attn_fwd_varlen_drop: " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);
    const int nqb = (T + LQB - 1) / LQB;
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, "attn_fwd_varlen_drop: grid too large");
    const dim3 grid((unsigned)(B * H * nqb));
    if (drop_p > 0.f)
        hipLaunchKernelGGL(attn_fwd_varlen_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)ctx, lse,
                           (const int*)klen, T, H, nqb, scale, drop_p, drop_seed);
    else
        hipLaunchKernelGGL(attn_fwd_varlen_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)ctx, lse,
                           (const int*)klen, T, H, nqb, scale, drop_p, drop_seed);
    return scl_check_launch("scl_attn_fwd_varlen_drop");
}

// workspace: scl_attn_long_ws_bytes(B, T, H) bytes (delta, f32 [B, H, T])
extern "C" int scl_attn_bwd_varlen(const void* qkv, const void* ctx, const void* dctx, const float* lse, const int32_t* klen, void* dqkv, void* ws,
                                   int B, int T, int H, int D, float scale, float drop_p, uint32_t drop_seed, void* stream) {
    SCL_REQUIRE(qkv && ctx && dctx && lse && klen && dqkv && ws && B > 0 && H > 0 && T >= 1 && drop_p >= 0.f && drop_p < 1.f,
                "attn_bwd_varlen: bad args");
    if (scl_attn_wide_takes(D))
        return scl_attn_wide_bwd(SCL_ROWS_PADDED, "scl_attn_bwd_varlen", qkv, ctx, dctx, lse, klen, dqkv, ws, B, T, H, D, 0, scale, drop_p, drop_seed,
                                 stream);
    SCL_REQUIRE(D == LD, "attn_bwd_varlen: " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);
    const int nqb = (T + LQB - 1) / LQB, nkw = (T + LKW - 1) / LKW;
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, "attn_bwd_varlen: grid too large");
    hipStream_t s = (hipStream_t)stream;
    float* delta = (float*)ws;
    const int64_t rows = (int64_t)B * T * H;
    hipLaunchKernelGGL(attn_delta_varlen_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, s, (const bf16_t*)ctx, (const bf16_t*)dctx,
                       delta, (const int*)klen, rows, T, H);
    int rc = scl_check_launch("scl_attn_bwd_varlen (delta)");
    if (rc) return rc;
#define ATT_BWD_VARLEN(DR)                                                                                                                        \
    hipLaunchKernelGGL(attn_bwd_dkdv_varlen_kernel<DR>, dim3((unsigned)(B * H * nkw)), dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dctx, \
                       lse, (const float*)delta, (bf16_t*)dqkv, (const int*)klen, T, H, nkw, scale, drop_p, drop_seed);                          \
    hipLaunchKernelGGL(attn_bwd_dq_varlen_kernel<DR>, dim3((unsigned)(B * H * nqb)), dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dctx,   \
                       lse, (const float*)delta, (bf16_t*)dqkv, (const int*)klen, T, H, nqb, scale, drop_p, drop_seed)
    if (drop_p > 0.f) { ATT_BWD_VARLEN(true); }
    else { ATT_BWD_VARLEN(false); }
#undef ATT_BWD_VARLEN
    return scl_check_launch("scl_attn_bwd_varlen");
}

extern "C" int scl_softmax_fwd_f32_varlen(const float* S, float* P, const int32_t* klen, int64_t R, int rows_per_utt, int T, int ldS, int Tp,
                                          void* stream) {
    SCL_REQUIRE(S && P && klen && R > 0 && rows_per_utt > 0 && R % rows_per_utt == 0 && T > 0 && Tp >= T && ldS >= T && (Tp & 3) == 0,
                "softmax_fwd_f32_varlen: need R %% rows_per_utt == 0, T <= Tp, T <= ldS, Tp %% 4 == 0");
    const dim3 grid((unsigned)((R + 3) / 4));
    if (Tp <= 64 * MAXV)
        hipLaunchKernelGGL(softmax_fwd_f32_varlen_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, S, P, (const int*)klen, R, rows_per_utt, T, ldS, Tp);
    else
        hipLaunchKernelGGL(softmax_fwd_f32_varlen_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, S, P, (const int*)klen, R, rows_per_utt, T, ldS, Tp);
    return scl_check_launch("scl_softmax_fwd_f32_varlen");
}

extern "C" int scl_zero_tail_rows(void* x, int is_f32, const int32_t* len, int B, int T, int C, void* stream) {
    SCL_REQUIRE(x && len && B > 0 && T > 0 && C > 0 && (C & 7) == 0, "zero_tail_rows: need C %% 8 == 0");
    const int vec_per_row = is_f32 ? C / 4 : C / 8;
    const int64_t n = (int64_t)B * T * vec_per_row;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(zero_tail_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (uint4*)x, (const int*)len, B, T, vec_per_row);
    return scl_check_launch("scl_zero_tail_rows");
}

extern "C" int scl_meanpool_fwd_varlen(const void* h, float* emb, const int32_t* len, int B, int T, int C, void* stream) {
    SCL_REQUIRE(h && emb && len && B > 0 && T > 0 && C > 0, "meanpool_fwd_varlen: bad args");
    hipLaunchKernelGGL(meanpool_fwd_varlen_kernel<bf16_t>, dim3(B), dim3(512), 0, (hipStream_t)stream, (const bf16_t*)h, emb, (const int*)len, T, C);
    return scl_check_launch("scl_meanpool_fwd_varlen");
}

extern "C" int scl_meanpool_fwd_varlen_f32(const float* h, float* emb, const int32_t* len, int B, int T, int C, void* stream) {
    SCL_REQUIRE(h && emb && len && B > 0 && T > 0 && C > 0, "meanpool_fwd_varlen_f32: bad args");
    hipLaunchKernelGGL(meanpool_fwd_varlen_kernel<float>, dim3(B), dim3(512), 0, (hipStream_t)stream, h, emb, (const int*)len, T, C);
    return scl_check_launch("scl_meanpool_fwd_varlen_f32");
}

static unsigned mp_bwd_grid(int64_t n) { const int64_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

extern "C" int scl_meanpool_bwd_varlen(const float* demb, const void* pre, void* dpre, const int32_t* len, int B, int T, int C, int ract,
                                       float drop_p, uint32_t seed, void* stream) {
    SCL_REQUIRE(demb && pre && dpre && len && B > 0 && T > 0 && C > 0 && drop_p >= 0.f && drop_p < 1.f, "meanpool_bwd_varlen: bad args");
    hipLaunchKernelGGL(meanpool_bwd_varlen_kernel<bf16_t>, dim3(mp_bwd_grid((int64_t)B * T * C)), dim3(256), 0, (hipStream_t)stream, demb,
                       (const bf16_t*)pre, (bf16_t*)dpre, (const int*)len, B, T, C, ract, drop_p, seed);
    return scl_check_launch("scl_meanpool_bwd_varlen");
}

extern "C" int scl_meanpool_bwd_varlen_f32(const float* demb, const float* pre, float* dpre, const int32_t* len, int B, int T, int C, int ract,
                                           float drop_p, uint32_t seed, void* stream) {
    SCL_REQUIRE(demb && pre && dpre && len && B > 0 && T > 0 && C > 0 && drop_p >= 0.f && drop_p < 1.f, "meanpool_bwd_varlen_f32: bad args");
    hipLaunchKernelGGL(meanpool_bwd_varlen_kernel<float>, dim3(mp_bwd_grid((int64_t)B * T * C)), dim3(256), 0, (hipStream_t)stream, demb, pre,
                       dpre, (const int*)len, B, T, C, ract, drop_p, seed);
    return scl_check_launch("scl_meanpool_bwd_varlen_f32");
}
