// attention_varlen.hip — a zero-padded batch of utterances of different lengths: per-utterance frame counts klen[b] (int32 on the
// device, 1 <= klen[b] <= T) play the part of fairseq's padding_mask, for scoring and for training.
//
//   scl_attn_fwd_varlen          the streaming forward of attention_long.hip with the key loop, the K / V staging and the last block's
//                                mask running to klen[b] instead of T: keys >= klen[b] are never loaded, and a block of 64 queries that
//                                starts at or beyond klen[b] writes zeros and leaves before the first barrier.  klen[b] is one value per
//                                workgroup, so the trip count and the early exit are workgroup-uniform.  Per query the blocks are visited
//                                in the order of scl_attn_fwd_long at T = klen[b]: rows < klen[b] carry the same bits.
//   scl_attn_fwd_varlen_drop     the same with attention dropout: keep-mask hash(seed, ((b*H + h)*T + q)*T + k) with the PADDED T, the
//                                index of the fixed-length kernels.
//   scl_attn_bwd_varlen          the deterministic streaming backward of attention_long.hip (delta, dK / dV per 128 keys, dQ per 64
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
#include "attn_tiles.h"

namespace {

constexpr int LD = 64;        // head dim
constexpr int LKB = 64;       // keys per streamed block
constexpr int LQB = 64;       // queries per workgroup
constexpr int LKW = 128;      // keys per workgroup (dK / dV)

__device__ __forceinline__ int clamp_len(int n, int T) { return n < 1 ? 1 : (n > T ? T : n); }

// attn_fwd_long_kernel with Tb = klen[b] keys (see attention_long.hip for the tile scheme)
template <bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_varlen_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, float* __restrict__ lse,
                                                              const int* __restrict__ klen, int T, int H, int nqb, float scale,
                                                              float drop_p, uint32_t drop_seed) {
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
    const uint64_t rowbase = (((uint64_t)b * H + h) * T + (uint64_t)(q < T ? q : 0)) * (uint64_t)T;      // mask index: the padded T
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
        if (DROP) {      // the sum above is of the undropped probabilities; P x mask feeds P V
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int key = key0 + 16 * t + 4 * g + rr;
                    s[t][rr] *= dropout_scale(drop_seed, rowbase + (uint64_t)(key < T ? key : 0), drop_p);
                }
        }
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

// =====================================================================================================================================
// Backward: the three passes of scl_attn_bwd_long with Tb = klen[b] (see attention_long.hip for the tile scheme)
// =====================================================================================================================================
// delta[(b*H + h)*T + q] = <dO, O> of the row for q < klen[b], 0 beyond (those rows of ctx / dctx are not read)
__global__ __launch_bounds__(256) void attn_delta_varlen_kernel(const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx,
                                                                float* __restrict__ delta, const int* __restrict__ klen, int64_t rows, int T, int H) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid >> 3;      // (b, q, h) in memory order
    const int c = (int)(gid & 7);
    const int64_t bq = row / H;
    const int h = (int)(row % H);
    const int64_t b = bq / T, q = bq % T;
    float dot = 0.f;
    if (row < rows && q < clamp_len(klen[b], T)) {
        const uint4 vo = *reinterpret_cast<const uint4*>(dctx + row * LD + 8 * c);
        const uint4 vc = *reinterpret_cast<const uint4*>(ctx + row * LD + 8 * c);
        const unsigned ow[4] = {vo.x, vo.y, vo.z, vo.w}, cw[4] = {vc.x, vc.y, vc.z, vc.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dot += __uint_as_float(ow[k] << 16) * __uint_as_float(cw[k] << 16);
            dot += __uint_as_float(ow[k] & 0xFFFF0000u) * __uint_as_float(cw[k] & 0xFFFF0000u);
        }
    }
    dot = lanes8_sum(dot);
    if (row < rows && c == 0) delta[(b * H + h) * T + q] = dot;
}

// ---- dK / dV: attn_bwd_dkdv_long_kernel over the utterance's own queries and keys -----------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_varlen_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   bf16_t* __restrict__ dqkv, const int* __restrict__ klen, int T, int H, int nkw,
                                                                   float scale, float drop_p, uint32_t drop_seed) {
    __shared__ __attribute__((aligned(16))) char smem[2][QT_BYTES];
    const int E = H * LD;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nkw, kblk = blockIdx.x % nkw;
    const int b = bh / H, h = bh % H;
    const int Tb = clamp_len(klen[b], T);      // one value per workgroup
    const bf16_t* base = qkv + (int64_t)b * T * pitch + h * LD;
    const bf16_t* dob = dctx + (int64_t)b * T * E + h * LD;
    const float* lse_bh = lse + ((int64_t)b * H + h) * T;
    const float* del_bh = delta + ((int64_t)b * H + h) * T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int key_w = kblk * LKW + 32 * wave;      // first of this wave's 32 keys
    if (kblk * LKW >= Tb) {      // the whole key block is padding: zero dK / dV rows, and out before any barrier (uniform: kblk and Tb are)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int key = key_w + 16 * j + lc;
            if (key < T) {
                bf16_t* dst = dqkv + ((int64_t)b * T + key) * pitch + h * LD + 4 * g;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    *reinterpret_cast<uint2*>(dst + E + 16 * dt) = make_uint2(0u, 0u);
                    *reinterpret_cast<uint2*>(dst + 2 * E + 16 * dt) = make_uint2(0u, 0u);
                }
            }
        }
        return;
    }
    // the wave's K / V rows as B operands (lane: key key_w + 16 j + lc, d = 32 ks + 8 g + 0..7)
    bf16x8 kf[2][2], vf[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        l_load_rows(base + E, pitch, key_w + 16 * j + lc, Tb, g, kf[j]);
        l_load_rows(base + 2 * E, pitch, key_w + 16 * j + lc, Tb, g, vf[j]);
    }
    const int nqt = (Tb + 31) / 32;
    QRegs r;
    qt_fetch(r, base, pitch, dob, E, lse_bh, del_bh, 0, Tb);
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
        if (u + 1 < nqt) qt_fetch(r, base, pitch, dob, E, lse_bh, del_bh, 32 * (u + 1), Tb);
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
                    const float pv = key >= Tb ? 0.f : __builtin_amdgcn_exp2f(__builtin_fmaf(sv[rr], sc2, -lq[a][rr]));      // rows past Tb: lse = huge -> 0
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
    // dK^T / dV^T: lane holds key key_w + 16 j + lc, d = 16 dt + 4 g + 0..3; keys of the block at or beyond Tb: zeros
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int key = key_w + 16 * j + lc;
        if (key < T) {
            const bool valid = key < Tb;
            bf16_t* dst = dqkv + ((int64_t)b * T + key) * pitch + h * LD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                *reinterpret_cast<uint2*>(dst + E + 16 * dt) = valid ? make_uint2(pack_bf2(dKt[dt][j][0] * scale, dKt[dt][j][1] * scale),
                                                                                  pack_bf2(dKt[dt][j][2] * scale, dKt[dt][j][3] * scale))
                                                                     : make_uint2(0u, 0u);
                *reinterpret_cast<uint2*>(dst + 2 * E + 16 * dt) = valid ? make_uint2(pack_bf2(dVt[dt][j][0], dVt[dt][j][1]), pack_bf2(dVt[dt][j][2], dVt[dt][j][3]))
                                                                         : make_uint2(0u, 0u);
            }
        }
    }
}

// ---- dQ: attn_bwd_dq_long_kernel over the utterance's own keys ---------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_varlen_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16_t* __restrict__ dqkv, const int* __restrict__ klen, int T, int H, int nqb,
                                                                 float scale, float drop_p, uint32_t drop_seed) {
    __shared__ __attribute__((aligned(16))) char smem[2][3][LKB * 128];      // [buffer][K rows, K tr, V rows]
    const int E = H * LD;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const int Tb = clamp_len(klen[b], T);      // one value per workgroup
    const bf16_t* base = qkv + (int64_t)b * T * pitch + h * LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int q0 = qblk * LQB + 16 * wave, q = q0 + lc;
    bf16_t* dst = dqkv + ((int64_t)b * T + q) * pitch + h * LD + 4 * g;
    if (qblk * LQB >= Tb) {      // the whole query block is padding: zero dQ rows, and out before any barrier (uniform: qblk and Tb are)
        if (q < T) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<uint2*>(dst + 16 * dt) = make_uint2(0u, 0u);
        }
        return;
    }
    const int nkb = (Tb + LKB - 1) / LKB;
    bf16x8 qf[2], of[2];
    l_load_rows(base, pitch, q, Tb, g, qf);
    l_load_rows(dctx + (int64_t)b * T * E + h * LD, E, q, Tb, g, of);
    const int64_t rbh = ((int64_t)b * H + h) * T;
    const float lq = q < Tb ? lse[rbh + q] * LOG2E : 1e30f;
    const float dl = q < Tb ? delta[rbh + q] : 0.f;
    KVRegs r;
    kv_fetch(r, base, pitch, E, 0, Tb);
    kv_store(r, smem[0][0], smem[0][1], smem[0][2], nullptr);
    __syncthreads();
    const float sc2 = scale * LOG2E;
    const uint64_t rowbase = ((uint64_t)rbh + (uint64_t)(q < T ? q : 0)) * (uint64_t)T;      // mask index: the padded T
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
        const int p = kb & 1;
        if (kb + 1 < nkb) kv_fetch(r, base, pitch, E, (kb + 1) * LKB, Tb);
        const char* Kr = smem[p][0];
        const char* Kt = smem[p][1];
        const char* Vr = smem[p][2];
        const int key0 = kb * LKB;
        f32x4 ds[4];      // dS^T[key = 16t + 4g + r][q = lc]
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_rows(Kr, t, ks, lane), qf[ks], sv, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_rows(Vr, t, ks, lane), of[ks], dp, 0, 0, 0);
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int key = key0 + 16 * t + 4 * g + rr;
                const float pv = key >= Tb ? 0.f : __builtin_amdgcn_exp2f(__builtin_fmaf(sv[rr], sc2, -lq));
                const float mk = DROP ? dropout_scale(drop_seed, rowbase + (uint64_t)(key < T ? key : 0), drop_p) : 1.f;
                ds[t][rr] = pv * (dp[rr] * mk - dl);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bf16x8 sf = l_pack8(ds[2 * u], ds[2 * u + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_tr(Kt, 32 * u, 32 * u + 16, dt, lane), sf, dq[dt], 0, 0, 0);
        }
        if (kb + 1 < nkb) kv_store(r, smem[p ^ 1][0], smem[p ^ 1][1], smem[p ^ 1][2], nullptr);
        __syncthreads();
    }
    if (q < T) {
        const bool valid = q < Tb;      // padded query rows of the last valid block: zeros, as the blocks beyond it
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<uint2*>(dst + 16 * dt) = valid ? make_uint2(pack_bf2(dq[dt][0] * scale, dq[dt][1] * scale), pack_bf2(dq[dt][2] * scale, dq[dt][3] * scale))
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
    SCL_REQUIRE(D == LD, "attn_fwd_varlen: needs head dim 64 (got D=%d)", D);
    const int nqb = (T + LQB - 1) / LQB;
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, "attn_fwd_varlen: grid too large");
    hipLaunchKernelGGL(attn_fwd_varlen_kernel<false>, dim3((unsigned)(B * H * nqb)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv,
                       (bf16_t*)ctx, lse, (const int*)klen, T, H, nqb, scale, 0.f, 0u);
    return scl_check_launch("scl_attn_fwd_varlen");
}

extern "C" int scl_attn_fwd_varlen_drop(const void* qkv, void* ctx, float* lse, const int32_t* klen, int B, int T, int H, int D, float scale,
                                        float drop_p, uint32_t drop_seed, void* stream) {
    SCL_REQUIRE(qkv && ctx && lse && klen && B > 0 && H > 0 && T >= 1 && drop_p >= 0.f && drop_p < 1.f, "attn_fwd_varlen_drop: bad args");
    SCL_REQUIRE(D == LD, "attn_fwd_varlen_drop: needs head dim 64 (got D=%d)", D);
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
    SCL_REQUIRE(D == LD, "attn_bwd_varlen: needs head dim 64 (got D=%d)", D);
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
