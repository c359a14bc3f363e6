// attention_long.hip — the fixed-length layout of the streaming attention (every utterance has T frames, T >= 1): forward, backward, and
// the looped fp32 row soft-max of the fp32 scoring path.  The encoder routes here above the 512 frames the materialised-score path
// (attention.hip: a whole score row in registers) accepts; nothing of size T^2 is written to memory.
//
// Head dim 64 is compiled here; the entries hand head dims 72..128 to attention_wide.hip (the same bodies with a padded head dim).
// The forward, delta and dQ kernels are the bodies of attn_stream_body.h (the tile scheme, the operand layouts and the dropout mask index are
// described there) with Rows::Fixed: utterance b at rows b*T, Tb = T, no length array.  attention_varlen.hip and attention_packed.hip hold
// the same bodies for a zero-padded and a packed variable-length batch.  The dK / dV kernel has a body of its own here.
#include "attn_stream_body.h"
#include "attn_wide.h"      // head dims 72..128: attention_wide.hip

namespace {

template <bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_long_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, float* __restrict__ lse,
                                                            int T, int H, int nqb, float scale, float drop_p, uint32_t drop_seed) {
    attn_stream_fwd_body<DROP, Rows::Fixed>(qkv, ctx, lse, nullptr, T, H, nqb, 0, 0, scale, drop_p, drop_seed);
}

__global__ __launch_bounds__(256) void attn_delta_kernel(const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx, float* __restrict__ delta,
                                                         int64_t rows, int T, int H) {
    attn_stream_delta_body<Rows::Fixed>(ctx, dctx, delta, nullptr, rows, T, H, 0);
}

// dK / dV: attn_stream_dkdv_body's scheme with Tb = T and no early exit, written out because the shared body compiles to a slower
// schedule for this layout (profiles/attn_stream_unify.txt).  A change to the tile scheme has to be made in both.
template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_long_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16_t* __restrict__ dqkv, int T, int H, int nkw, float scale,
                                                                 float drop_p, uint32_t drop_seed) {
    __shared__ __attribute__((aligned(16))) char smem[2][QT_BYTES];
    const int E = H * LD;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nkw, kblk = blockIdx.x % nkw;
    const int b = bh / H, h = bh % H;
    const bf16_t* base = qkv + (int64_t)b * T * pitch + h * LD;
    const bf16_t* dob = dctx + (int64_t)b * T * E + h * LD;
    const float* lse_bh = lse + ((int64_t)b * H + h) * T;
    const float* del_bh = delta + ((int64_t)b * H + h) * T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int key_w = kblk * LKW + 32 * wave;      // first of this wave's 32 keys
    // the wave's K / V rows as B operands (lane: key key_w + 16 j + lc, d = 32 ks + 8 g + 0..7)
    bf16x8 kf[2][2], vf[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        l_load_rows(base + E, pitch, key_w + 16 * j + lc, T, g, kf[j]);
        l_load_rows(base + 2 * E, pitch, key_w + 16 * j + lc, T, g, vf[j]);
    }
    const int nqt = (T + 31) / 32;
    QRegs r;
    qt_fetch(r, base, pitch, dob, E, lse_bh, del_bh, 0, T);
    qt_store(r, smem[0]);
    __syncthreads();
    f32x4 dVt[4][2], dKt[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { dVt[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; dKt[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const float sc2 = scale * LOG2E;
    for (int u = 0; u < nqt; ++u) {
        const int p = u & 1;
        if (u + 1 < nqt) qt_fetch(r, base, pitch, dob, E, lse_bh, del_bh, 32 * (u + 1), T);
        const char* Qk = smem[p];
        const char* Qt = Qk + 4096;
        const char* Ok = Qk + 8192;
        const char* Ot = Qk + 12288;
        const float* lsP = reinterpret_cast<const float*>(Qk + 16384);
        const float* dlP = lsP + 32;
        bf16x8 qa[2][2], oa[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) { qa[a][ks] = l_frag_rows(Qk, a, ks, lane); oa[a][ks] = l_frag_rows(Ok, a, ks, lane); }
        float lq[2][4], dq_[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float4 l4 = *reinterpret_cast<const float4*>(lsP + 16 * a + 4 * g), d4 = *reinterpret_cast<const float4*>(dlP + 16 * a + 4 * g);
            lq[a][0] = l4.x; lq[a][1] = l4.y; lq[a][2] = l4.z; lq[a][3] = l4.w;
            dq_[a][0] = d4.x; dq_[a][1] = d4.y; dq_[a][2] = d4.z; dq_[a][3] = d4.w;
        }
        f32x4 P[2][2], dS[2][2];      // [query tile a][key tile j]: D[q = 16a + 4g + r][key = 16j + lc]
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int key = key_w + 16 * j + lc;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
                sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[a][0], kf[j][0], sv, 0, 0, 0);
                sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[a][1], kf[j][1], sv, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa[a][0], vf[j][0], dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa[a][1], vf[j][1], dp, 0, 0, 0);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int qq = 32 * u + 16 * a + 4 * g + rr;
                    const float pv = key >= T ? 0.f : __builtin_amdgcn_exp2f(__builtin_fmaf(sv[rr], sc2, -lq[a][rr]));      // rows past T: lse = huge -> 0
                    const float mk = DROP ? dropout_scale(drop_seed, (((uint64_t)b * H + h) * T + (uint64_t)(qq < T ? qq : 0)) * (uint64_t)T +
                                                                         (uint64_t)(key < T ? key : 0), drop_p) : 1.f;
                    P[a][j][rr] = pv * mk;
                    dS[a][j][rr] = pv * (dp[rr] * mk - dq_[a][rr]);
                }
            }
        }
        bf16x8 pP[2], pS[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) { pP[j] = l_pack8(P[0][j], P[1][j]); pS[j] = l_pack8(dS[0][j], dS[1][j]); }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const bf16x8 ot = l_frag_tr(Ot, 0, 16, dt, lane);
            const bf16x8 qt = l_frag_tr(Qt, 0, 16, dt, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                dVt[dt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ot, pP[j], dVt[dt][j], 0, 0, 0);
                dKt[dt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, pS[j], dKt[dt][j], 0, 0, 0);
            }
        }
        if (u + 1 < nqt) qt_store(r, smem[p ^ 1]);
        __syncthreads();
    }
    // dK^T / dV^T: lane holds key key_w + 16 j + lc, d = 16 dt + 4 g + 0..3
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int key = key_w + 16 * j + lc;
        if (key < T) {
            bf16_t* dst = dqkv + ((int64_t)b * T + key) * pitch + h * LD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                *reinterpret_cast<uint2*>(dst + E + 16 * dt) = make_uint2(pack_bf2(dKt[dt][j][0] * scale, dKt[dt][j][1] * scale),
                                                                          pack_bf2(dKt[dt][j][2] * scale, dKt[dt][j][3] * scale));
                *reinterpret_cast<uint2*>(dst + 2 * E + 16 * dt) = make_uint2(pack_bf2(dVt[dt][j][0], dVt[dt][j][1]), pack_bf2(dVt[dt][j][2], dVt[dt][j][3]));
            }
        }
    }
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_long_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               bf16_t* __restrict__ dqkv, int T, int H, int nqb, float scale,
                                                               float drop_p, uint32_t drop_seed) {
    attn_stream_dq_body<DROP, Rows::Fixed>(qkv, dctx, lse, delta, dqkv, nullptr, T, H, nqb, 0, 0, scale, drop_p, drop_seed);
}

// fp32 row soft-max of any length: one wave per row
__global__ __launch_bounds__(256) void softmax_fwd_f32_long_kernel(const float* __restrict__ S, float* __restrict__ P, int64_t R, int T,
                                                                   int ldS, int Tp) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    softmax_f32_looped_row(S + row * ldS, P + row * Tp, T, Tp, threadIdx.x & 63);
}

}  // namespace

extern "C" int scl_attn_fwd_long(const void* qkv, void* ctx, float* lse, int B, int T, int H, int D, float scale, float drop_p,
                                 uint32_t drop_seed, void* stream) {
    SCL_REQUIRE(qkv && ctx && lse && B > 0 && H > 0 && T >= 1 && drop_p >= 0.f && drop_p < 1.f, "attn_fwd_long: bad args");
    if (scl_attn_wide_takes(D))
        return scl_attn_wide_fwd(SCL_ROWS_FIXED, "scl_attn_fwd_long", qkv, ctx, lse, nullptr, B, T, H, D, 0, scale, drop_p, drop_seed, stream);
    SCL_REQUIRE(D == LD, "attn_fwd_long: " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);
    const int nqb = (T + LQB - 1) / LQB;
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, "attn_fwd_long: grid too large");
    const dim3 grid((unsigned)(B * H * nqb));
    if (drop_p > 0.f)
        hipLaunchKernelGGL(attn_fwd_long_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)ctx, lse, T, H, nqb,
                           scale, drop_p, drop_seed);
    else
        hipLaunchKernelGGL(attn_fwd_long_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)ctx, lse, T, H, nqb,
                           scale, drop_p, drop_seed);
    return scl_check_launch("scl_attn_fwd_long");
}

extern "C" long long scl_attn_long_ws_bytes(int B, int T, int H) {
    if (B <= 0 || T <= 0 || H <= 0) return 0;
    return ((long long)B * H * T * 4 + 255) / 256 * 256;      // delta = rowsum(dO o O), f32 [B, H, T]
}

extern "C" int scl_attn_bwd_long(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, void* ws, int B, int T,
                                 int H, int D, float scale, float drop_p, uint32_t drop_seed, void* stream) {
    SCL_REQUIRE(qkv && ctx && dctx && lse && dqkv && ws && B > 0 && H > 0 && T >= 1 && drop_p >= 0.f && drop_p < 1.f, "attn_bwd_long: bad args");
    if (scl_attn_wide_takes(D))
        return scl_attn_wide_bwd(SCL_ROWS_FIXED, "scl_attn_bwd_long", qkv, ctx, dctx, lse, nullptr, dqkv, ws, B, T, H, D, 0, scale, drop_p, drop_seed,
                                 stream);
    SCL_REQUIRE(D == LD, "attn_bwd_long: " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);
    const int nqb = (T + LQB - 1) / LQB, nkw = (T + LKW - 1) / LKW;
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, "attn_bwd_long: grid too large");
    hipStream_t s = (hipStream_t)stream;
    float* delta = (float*)ws;
    const int64_t rows = (int64_t)B * T * H;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, s, (const bf16_t*)ctx, (const bf16_t*)dctx, delta,
                       rows, T, H);
    int rc = scl_check_launch("scl_attn_bwd_long (delta)");
    if (rc) return rc;
#define ATT_BWD_LONG(DR)                                                                                                                        \
    hipLaunchKernelGGL(attn_bwd_dkdv_long_kernel<DR>, dim3((unsigned)(B * H * nkw)), dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dctx, \
                       lse, (const float*)delta, (bf16_t*)dqkv, T, H, nkw, scale, drop_p, drop_seed);                                           \
    hipLaunchKernelGGL(attn_bwd_dq_long_kernel<DR>, dim3((unsigned)(B * H * nqb)), dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dctx,   \
                       lse, (const float*)delta, (bf16_t*)dqkv, T, H, nqb, scale, drop_p, drop_seed)
    if (drop_p > 0.f) { ATT_BWD_LONG(true); }
    else { ATT_BWD_LONG(false); }
#undef ATT_BWD_LONG
    return scl_check_launch("scl_attn_bwd_long");
}

extern "C" int scl_softmax_fwd_f32_long(const float* S, float* P, int64_t R, int T, int ldS, int Tp, void* stream) {
    SCL_REQUIRE(S && P && R > 0 && T > 0 && Tp >= T && ldS >= T && (Tp & 3) == 0, "softmax_fwd_f32_long: need T <= Tp, T <= ldS, Tp %% 4 == 0");
    hipLaunchKernelGGL(softmax_fwd_f32_long_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, S, P, R, T, ldS, Tp);
    return scl_check_launch("scl_softmax_fwd_f32_long");
}
