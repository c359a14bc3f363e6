// attn_stream_body.h — streaming ("flash") attention for head dim 64 and any clip length (T >= 1), forward and backward, as device-function
// bodies shared by the three row layouts of a batch (everything is internal to the including file and force-inlined into its kernels).
// Nothing of size T^2 is written to memory.
// Head dims 72..128 (XLS-R 1B: 80, 2B: 120) run the same scheme on a head dim padded to 96 or 128 in registers and LDS: attn_wide_body.h,
// compiled by attention_wide.hip, which takes Rows / UttRows / zero_tail_vectors and the block sizes from here.  The two sets of bodies are
// kept textually apart (templated on the padded head dim, the kernels of head dim 64 compiled to another schedule): a change to the
// tile scheme has to be made in both.
//
// Operands and outputs as scl_attn_fwd / scl_attn_bwd: qkv / dqkv bf16 [rows, 3, H, 64]; ctx / dctx bf16 [rows, H*64]; lse f32 [B, H, T]
// = log sum_k exp(scale * q.k).  Attention dropout draws keep-mask hash(seed, ((b*H + h)*T + q)*T + k), the index of the fused kernels
// and of scl_dropout_rows.  Every global offset is 64-bit.
//
// THE ROW LAYOUTS (template parameter Rows; utterance b owns Tb rows from row r0, see UttRows):
//   Rows::Fixed    attention_long.hip: every utterance has T frames.  r0 = b*T, Tb = T, `lens` is null and never read.  (Its dK / dV
//                  kernel is the one body not taken from here: attention_long.hip.)
//   Rows::Padded   attention_varlen.hip: the zero-padded rectangle.  Utterance b owns rows b*T .. b*T + T - 1 of qkv / ctx / dctx / dqkv,
//                  `lens` is klen[B]; rows >= klen[b] of a partial block are stored as zeros and a block beyond klen[b] writes zeros.
//   Rows::Packed   attention_packed.hip: valid frames back to back.  Utterance b owns rows row0[b] .. row0[b+1] - 1, `lens` is row0[B+1]
//                  and Mq the launch's row count.  The rows behind an utterance belong to the NEXT one (or to nobody), so nothing is
//                  stored at or beyond Tb and a block that starts there leaves before its first barrier without a store; the rows
//                  [row0[B], Mq) that belong to no utterance are written as zeros by every launch (zero_tail_vectors).
// lse, delta and the attention-dropout mask index live in the padded (b, h, q, T) space in every layout: the same batch draws the same
// masks and carries the same bits in each.  Tb is one value per workgroup, so the trip counts and the early exits are
// workgroup-uniform; per query the blocks are visited in the order of the fixed layout at T = Tb.
//
// THE TILE SCHEME.  Forward, one workgroup per (utterance, head, block of 64 queries), 4 waves of 16 queries.  Blocks of 64 keys stream
// through LDS (double-buffered, the next block's loads are issued before the current block is multiplied and written to LDS after it: one
// barrier per block).  Per block and wave:
//   S^T[key][q] = K Q^T       MFMA(A = K rows from LDS, B = the wave's Q rows held in registers)  -> lane owns ONE query (lc) and keys
//                             16t + 4g + r of each 16-key tile t: the row maximum is an in-lane max plus two cross-lane steps
//   online soft-max in fp32:  m' = max(m, rowmax), O *= 2^((m - m') scale log2 e), l = l * the same + rowsum(2^((S - m') scale log2 e))
//   O^T[d][q]  += V^T P^T     the exponentials, packed to bf16, ARE the B operand (the transposed LDS read of V supplies the permuted k)
// The rescale is applied on every block (no deferred rescale): the probabilities fed to the MFMA are <= 1 as in the fused kernel.
//
// Backward (P recomputed from lse, delta = rowsum(dO o O) by a small first kernel into the workspace):
//   dK / dV: one workgroup per (utterance, head, block of 128 keys); wave w owns keys 32w..32w+31 (their K / V fragments in registers,
//            dK^T / dV^T in accumulators) while the workgroup sweeps the queries 32 at a time (Q and dO tiles in LDS, row and
//            transposed images, double-buffered): S = Q K^T, dP = dO V^T, P = exp(scale S - lse), dS = P (dP mask - delta),
//            dV^T += dO^T (P mask), dK^T += Q^T dS.
//   dQ:      one workgroup per (utterance, head, block of 64 queries), as the forward: S^T = K Q^T, dP^T = V dO^T, dS^T as above,
//            dQ^T += K^T dS^T with K's transposed image.
// Each output element is summed by one wave in a fixed order: no atomics, bitwise reproducible.
//
// Also here: the looped fp32 row soft-max of the fp32 scoring path (softmax_f32_looped_row), one wave per row.
#pragma once
#include "attn_tiles.h"      // lk_off / lt_off tile images, l_frag_* / l_pack8 / l_load_rows operands, kv_fetch / kv_store / qt_fetch / qt_store staging

namespace {

constexpr int LD = 64;        // head dim
constexpr int LKB = 64;       // keys per streamed block (forward, dQ)
constexpr int LQB = 64;       // queries per workgroup (forward, dQ)
constexpr int LKW = 128;      // keys per workgroup (dK / dV)

enum class Rows { Fixed, Padded, Packed };

__device__ __forceinline__ int clamp_len(int n, int T) { return n < 1 ? 1 : (n > T ? T : n); }

// first row and frame count of utterance b.  Fixed: b*T and T, `lens` is not read.  Padded / packed: both clamped for memory safety (the
// host copy is validated before the upload): 1 <= Tb <= T, and in the packed layout 0 <= r0 and r0 + Tb <= Mq
template <Rows L>
struct UttRows {
    int64_t r0;
    int Tb;
    __device__ __forceinline__ UttRows(const int* __restrict__ lens, int b, int T, int Mq) {
        if constexpr (L == Rows::Packed) {
            const int a = lens[b];
            const int first = a < 0 ? 0 : (a > Mq - 1 ? Mq - 1 : a);
            const int n = clamp_len(lens[b + 1] - a, T);
            r0 = first;
            Tb = n > Mq - first ? Mq - first : n;
        } else {
            r0 = (int64_t)b * T;
            Tb = L == Rows::Fixed ? T : clamp_len(lens[b], T);
        }
    }
};

// packed layout: rows [lens[B], Mq) of x (row_vecs 16-byte vectors each) = 0, the launch's threads striding over them
__device__ __forceinline__ void zero_tail_vectors(uint4* __restrict__ x, const int* __restrict__ lens, int B, int Mq, int row_vecs) {
    const int last = lens[B];
    const int Mv = last < 0 ? 0 : (last > Mq ? Mq : last);
    const int64_t n = (int64_t)(Mq - Mv) * row_vecs;
    uint4* tail = x + (int64_t)Mv * row_vecs;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) tail[i] = make_uint4(0u, 0u, 0u, 0u);
}

// =====================================================================================================================================
// Forward
// =====================================================================================================================================
template <bool DROP, Rows L>
__device__ __forceinline__ void attn_stream_fwd_body(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, float* __restrict__ lse,
                                                     const int* __restrict__ lens, int T, int H, int nqb, int B, int Mq, float scale,
                                                     float drop_p, uint32_t drop_seed) {
    constexpr bool PACKED = L == Rows::Packed;
    __shared__ __attribute__((aligned(16))) char smem[2][2][LKB * 128];      // [buffer][K rows, V tr][64 keys x 128 B]
    const int E = H * LD;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const UttRows<L> utt(lens, b, T, Mq);
    const int Tb = utt.Tb;      // one value per workgroup: everything that depends on it is workgroup-uniform
    const bf16_t* base = qkv + utt.r0 * pitch + h * LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int q = qblk * LQB + 16 * wave + lc;
    bf16_t* dst = ctx + (utt.r0 + q) * E + h * LD + 4 * g;
    float* lse_q = lse + ((int64_t)b * H + h) * T + q;
    if constexpr (PACKED) zero_tail_vectors(reinterpret_cast<uint4*>(ctx), lens, B, Mq, E / 8);
    if constexpr (L != Rows::Fixed) {
        if (qblk * LQB >= Tb) {      // the whole query block is padding: zeros, and out before any barrier (uniform: qblk and Tb are)
            if (q < T) {
                if (g == 0) *lse_q = 0.f;      // lse is padded in every layout
                if constexpr (!PACKED) {       // packed: these rows are another utterance's
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<uint2*>(dst + 16 * dt) = make_uint2(0u, 0u);
                }
            }
            return;
        }
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
        const bool valid = q < Tb;      // padded query rows of the last valid block: zeros, as the blocks beyond it (packed: not stored)
        if (g == 0) *lse_q = valid ? scale * m + __logf(l) : 0.f;
        if (!PACKED || valid) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(dst + 16 * dt) = valid ? make_uint2(pack_bf2(o[dt][0] * inv, o[dt][1] * inv), pack_bf2(o[dt][2] * inv, o[dt][3] * inv))
                                                                 : make_uint2(0u, 0u);
        }
    }
}

// =====================================================================================================================================
// Backward
// =====================================================================================================================================
// delta[(b*H + h)*T + q] = <dO, O> of the row for q < Tb, 0 beyond (those rows of ctx / dctx are not read); one thread group of 8 per
// (b, q, h) of the PADDED space in every layout, rows = B * T * H (8 lanes per row, one 16-byte piece each, fixed-order sum)
template <Rows L>
__device__ __forceinline__ void attn_stream_delta_body(const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx, float* __restrict__ delta,
                                                       const int* __restrict__ lens, int64_t rows, int T, int H, int Mq) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid >> 3;      // (b, q, h) in memory order
    const int c = (int)(gid & 7);
    const int64_t bq = row / H;
    const int h = (int)(row % H);
    const int64_t b = bq / T, q = bq % T;
    float dot = 0.f;
    if (row < rows) {
        const UttRows<L> utt(lens, (int)b, T, Mq);
        if (L == Rows::Fixed || q < utt.Tb) {
            const int64_t src = L == Rows::Packed ? (utt.r0 + q) * H + h : row;
            const uint4 vo = *reinterpret_cast<const uint4*>(dctx + src * LD + 8 * c);
            const uint4 vc = *reinterpret_cast<const uint4*>(ctx + src * LD + 8 * c);
            const unsigned ow[4] = {vo.x, vo.y, vo.z, vo.w}, cw[4] = {vc.x, vc.y, vc.z, vc.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                dot += __uint_as_float(ow[k] << 16) * __uint_as_float(cw[k] << 16);
                dot += __uint_as_float(ow[k] & 0xFFFF0000u) * __uint_as_float(cw[k] & 0xFFFF0000u);
            }
        }
    }
    dot = lanes8_sum(dot);
    if (row < rows && c == 0) delta[(b * H + h) * T + q] = dot;
}

// ---- dK / dV ------------------------------------------------------------------------------------------------------------------------
// Query tiles of 32 rows per step: QRegs / qt_fetch / qt_store of attn_tiles.h (Q rows, Q tr, dO rows, dO tr images, lse x log2 e, delta)
template <bool DROP, Rows L>
__device__ __forceinline__ void attn_stream_dkdv_body(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      bf16_t* __restrict__ dqkv, const int* __restrict__ lens, int T, int H, int nkw, int Mq,
                                                      float scale, float drop_p, uint32_t drop_seed) {
    static_assert(L != Rows::Fixed, "the fixed layout's dK / dV kernel has its own body in attention_long.hip");
    constexpr bool PACKED = L == Rows::Packed;
    __shared__ __attribute__((aligned(16))) char smem[2][QT_BYTES];
    const int E = H * LD;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nkw, kblk = blockIdx.x % nkw;
    const int b = bh / H, h = bh % H;
    const UttRows<L> utt(lens, b, T, Mq);
    const int Tb = utt.Tb;      // one value per workgroup
    const bf16_t* base = qkv + utt.r0 * pitch + h * LD;
    const bf16_t* dob = dctx + utt.r0 * E + h * LD;
    const float* lse_bh = lse + ((int64_t)b * H + h) * T;
    const float* del_bh = delta + ((int64_t)b * H + h) * T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int key_w = kblk * LKW + 32 * wave;      // first of this wave's 32 keys
    if (kblk * LKW >= Tb) {      // the whole key block is padding: zero dK / dV rows, and out before any barrier (uniform: kblk and Tb are)
        if constexpr (PACKED) return;      // packed: these rows are another utterance's
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int key = key_w + 16 * j + lc;
            if (key < T) {
                bf16_t* dst = dqkv + (utt.r0 + key) * pitch + h * LD + 4 * g;
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
        if (key < (PACKED ? Tb : T)) {      // packed: nothing is stored at or beyond Tb
            const bool valid = key < Tb;
            bf16_t* dst = dqkv + (utt.r0 + key) * pitch + h * LD + 4 * g;
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

// ---- dQ -------------------------------------------------------------------------------------------------------------------------------
template <bool DROP, Rows L>
__device__ __forceinline__ void attn_stream_dq_body(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                    const float* __restrict__ lse, const float* __restrict__ delta,
                                                    bf16_t* __restrict__ dqkv, const int* __restrict__ lens, int T, int H, int nqb, int B, int Mq,
                                                    float scale, float drop_p, uint32_t drop_seed) {
    constexpr bool PACKED = L == Rows::Packed;
    __shared__ __attribute__((aligned(16))) char smem[2][3][LKB * 128];      // [buffer][K rows, K tr, V rows]
    const int E = H * LD;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const UttRows<L> utt(lens, b, T, Mq);
    const int Tb = utt.Tb;      // one value per workgroup
    const bf16_t* base = qkv + utt.r0 * pitch + h * LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int q0 = qblk * LQB + 16 * wave, q = q0 + lc;
    bf16_t* dst = dqkv + (utt.r0 + q) * pitch + h * LD + 4 * g;
    if constexpr (PACKED) zero_tail_vectors(reinterpret_cast<uint4*>(dqkv), lens, B, Mq, 3 * E / 8);
    if constexpr (L != Rows::Fixed) {
        if (qblk * LQB >= Tb) {      // the whole query block is padding: zero dQ rows, and out before any barrier (uniform: qblk and Tb are)
            if constexpr (PACKED) return;      // packed: these rows are another utterance's
            if (q < T) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<uint2*>(dst + 16 * dt) = make_uint2(0u, 0u);
            }
            return;
        }
    }
    const int nkb = (Tb + LKB - 1) / LKB;
    bf16x8 qf[2], of[2];
    l_load_rows(base, pitch, q, Tb, g, qf);
    l_load_rows(dctx + utt.r0 * E + h * LD, E, q, Tb, g, of);
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
    if (q < (PACKED ? Tb : T)) {      // packed: nothing is stored at or beyond Tb
        const bool valid = q < Tb;      // padded query rows of the last valid block: zeros, as the blocks beyond it
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<uint2*>(dst + 16 * dt) = valid ? make_uint2(pack_bf2(dq[dt][0] * scale, dq[dt][1] * scale), pack_bf2(dq[dt][2] * scale, dq[dt][3] * scale))
                                                             : make_uint2(0u, 0u);
    }
}

// =====================================================================================================================================
// fp32 row soft-max of any length by one wave: a looped online (max, sum) pass over the first Tv columns of s, then the write pass
// (p[c] = 0 for Tv <= c < Tp)
// =====================================================================================================================================
__device__ __forceinline__ void softmax_f32_looped_row(const float* s, float* p, int Tv, int Tp, int lane) {
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

}  // namespace
