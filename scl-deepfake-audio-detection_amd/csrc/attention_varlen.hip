// attention_varlen.hip — scoring a zero-padded batch of utterances of different lengths: per-utterance frame counts klen[b] (int32 on the
// device, 1 <= klen[b] <= T) play the part of fairseq's padding_mask.  Forward only, no dropout (scoring runs in eval mode under no_grad).
//
//   scl_attn_fwd_varlen          the streaming forward of attention_long.hip with the key loop, the K / V staging and the last block's
//                                mask running to klen[b] instead of T: keys >= klen[b] are never loaded, and a block of 64 queries that
//                                starts at or beyond klen[b] writes zeros and leaves before the first barrier.  klen[b] is one value per
//                                workgroup, so the trip count and the early exit are workgroup-uniform.  Per query the blocks are visited
//                                in the order of scl_attn_fwd_long at T = klen[b]: rows < klen[b] carry the same bits.
//   scl_softmax_fwd_f32_varlen   the fp32 row soft-max of the fp32 scoring path over the first klen[row / rows_per_utt] columns (row in
//                                registers up to 512 columns, looped above); every other column up to Tp is written as 0.
//   scl_zero_tail_rows           x[b][t >= len[b]][:] = 0 (fairseq's index_put(x, padding_mask, 0) after post_extract_proj; feats tail).
//   scl_meanpool_fwd_varlen      emb[b] = sum_{t < len[b]} h[b][t] / len[b], the summation order of scl_meanpool_fwd.
// The device-side counts are clamped to [1, T] for memory safety; scl_varlen_check_lengths validates the host copy before the upload.
#include "attn_tiles.h"

namespace {

constexpr int LD = 64;        // head dim
constexpr int LKB = 64;       // keys per streamed block
constexpr int LQB = 64;       // queries per workgroup
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ int clamp_len(int n, int T) { return n < 1 ? 1 : (n > T ? T : n); }

// attn_fwd_long_kernel<false> with Tb = klen[b] keys (see attention_long.hip for the tile scheme)
__global__ __launch_bounds__(256) void attn_fwd_varlen_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, float* __restrict__ lse,
                                                              const int* __restrict__ klen, int T, int H, int nqb, float scale) {
    __shared__ __attribute__((aligned(16))) char smem[2][2][LKB * 128];      // [buffer][K rows, V tr][64 keys x 128 B]
    const int E = H * LD;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const int Tb = clamp_len(klen[b], T);      // one value per workgroup: everything that depends on it is workgroup-uniform
    const bf16_t* base = qkv + (int64_t)b * T * pitch + h * LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int q = qblk * LQB + 16 * wave + lc;
    bf16_t* dst = ctx + ((int64_t)b * T + q) * E + h * LD + 4 * g;
    float* lse_q = lse + ((int64_t)b * H + h) * T + q;
    if (qblk * LQB >= Tb) {      // the whole query block is padding: zeros, and out before any barrier (uniform: qblk and Tb are)
        if (q < T) {
            if (g == 0) *lse_q = 0.f;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<uint2*>(dst + 16 * dt) = make_uint2(0u, 0u);
        }
        return;
    }
    const int nkb = (Tb + LKB - 1) / LKB;
    bf16x8 qf[2];
    l_load_rows(base, pitch, q, Tb, g, qf);
    KVRegs r;
    kv_fetch(r, base, pitch, E, 0, Tb);
    kv_store(r, smem[0][0], nullptr, nullptr, smem[0][1]);
    __syncthreads();
    const float sl2 = scale * LOG2E;
    float m = -INFINITY, l = 0.f;      // running max (raw score units) and this lane's share of the running sum
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
        const int p = kb & 1;
        if (kb + 1 < nkb) kv_fetch(r, base, pitch, E, (kb + 1) * LKB, Tb);      // in flight under this block's products
        const char* Kr = smem[p][0];
        const char* Vt = smem[p][1];
        const int key0 = kb * LKB;
        f32x4 s[4];
        float mb = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_rows(Kr, t, ks, lane), qf[ks], s[t], 0, 0, 0);
            if (key0 + LKB > Tb) {      // the last block only
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    if (key0 + 16 * t + 4 * g + rr >= Tb) s[t][rr] = -INFINITY;
            }
            mb = fmaxf(mb, fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])));
        }
        mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
        mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
        const float mn = fmaxf(m, mb);      // finite: every block holds at least one key < Tb
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * sl2);      // 0 on the first block (m = -inf)
        m = mn;
        const float msl = -mn * sl2;
        float ls = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) { s[t][rr] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][rr], sl2, msl)); ls += s[t][rr]; }
        l = l * alpha + ls;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bf16x8 pf = l_pack8(s[2 * u], s[2 * u + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_tr(Vt, 32 * u, 32 * u + 16, dt, lane), pf, o[dt], 0, 0, 0);
        }
        if (kb + 1 < nkb) kv_store(r, smem[p ^ 1][0], nullptr, nullptr, smem[p ^ 1][1]);      // its last readers finished before the previous barrier
        __syncthreads();
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    if (q < T) {
        const bool valid = q < Tb;      // padded query rows of the last valid block: zeros, as the blocks beyond it
        if (g == 0) *lse_q = valid ? scale * m + __logf(l) : 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<uint2*>(dst + 16 * dt) = valid ? make_uint2(pack_bf2(o[dt][0] * inv, o[dt][1] * inv), pack_bf2(o[dt][2] * inv, o[dt][3] * inv))
                                                             : make_uint2(0u, 0u);
    }
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
    } else {      // attention_long.hip's softmax_fwd_f32_long_kernel: online (max, sum) pass, then the write pass
        float m = -INFINITY, l = 0.f;
        for (int c = lane; c < Tv; c += 64) {
            const float v = s[c];
            if (v > m) { l = l * __expf(m - v) + 1.f; m = v; }
            else if (m != -INFINITY) l += __expf(v - m);      // v = m = -inf adds nothing
        }
        const float mx = wave_max(m);
        const float sum = wave_sum(m == -INFINITY ? 0.f : l * __expf(m - mx));
        const float inv = 1.0f / sum;
        for (int c = lane; c < Tp; c += 64) p[c] = c < Tv ? __expf(s[c] - mx) * inv : 0.f;
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
    SCL_REQUIRE(D == LD, "attn_fwd_varlen: needs head dim 64 (got D=%d)", D);
    const int nqb = (T + LQB - 1) / LQB;
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, "attn_fwd_varlen: grid too large");
    hipLaunchKernelGGL(attn_fwd_varlen_kernel, dim3((unsigned)(B * H * nqb)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)ctx,
                       lse, (const int*)klen, T, H, nqb, scale);
    return scl_check_launch("scl_attn_fwd_varlen");
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
