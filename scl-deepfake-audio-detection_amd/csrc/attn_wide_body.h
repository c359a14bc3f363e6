// attn_wide_body.h — the streaming attention bodies of attn_stream_body.h for head dims 72..128 (D % 8 == 0), on a PADDED head dim DP:
// DP = 96 serves D = 72..96, DP = 128 serves D = 104..128.  Same tile scheme, same row layouts (Rows / UttRows of attn_stream_body.h), same
// lse, delta workspace, dropout mask index, early exits, zero rows and fixed summation order; read the comment block there first.  The
// head-dim-64 bodies and their tile helpers stay textually apart in attn_stream_body.h / attn_tiles.h: templating them on DP compiled to
// a different instruction schedule for head dim 64.  A change to the tile scheme has to be made in both.  Everything here is internal
// to the including file (attention_wide.hip).
//
// WHAT THE PADDING MEANS.  In memory a head is D columns wide.  Columns D..DP-1 of a head's row are the next head's data (for the last
// head the next section's or the next row's, or they lie past the buffer): they are never read and never written.  A 16-byte chunk c of
// a q / k / v / dctx row is loaded when 8 c < D and is zero in registers and LDS otherwise; zero columns add 0 to Q K^T and dO V^T; an
// output group of 4 columns 16 dt + 4 g is stored when it lies below D; the last 16-column tile of O / dQ / dK / dV gets no MFMA when
// it lies at or beyond D (D <= 80 at DP = 96, D <= 112 at DP = 128: workgroup-uniform).  The k step of Q K^T that holds column D may be
// part zeros (half of it at D = 80).
//
// LDS per workgroup (DP = 96 / 128): forward 2 x 2 x 64 x 2 DP B = 48 / 64 KiB; dQ 2 x 3 x 64 x 2 DP B = 72 / 96 KiB; dK / dV
// 2 x (4 x 32 x 2 DP + 256) B = 48.5 / 64.5 KiB, with 8 DP / 8 accumulator and DP / 2 K / V fragment registers per lane.
#pragma once
#include "attn_stream_body.h"      // Rows, UttRows, zero_tail_vectors, LKB / LQB / LKW; attn_tiles.h: l_pack8, LOG2E

namespace {
namespace wide {      // the names of attn_tiles.h / attn_stream_body.h, with the padded head dim as a template parameter

// LDS images of a [rows][DP] bf16 tile, rows of 2 DP bytes.  Row image for ds_read_b128 row reads (l_frag_rows: lane = row 16 rb +
// (lane & 15), 16-byte slot 4 ks + (lane >> 4)), tr image for ds_read_b64_tr_b16 (l_frag_tr: four lanes read one 32-byte chunk of a row,
// 8-byte aligned, every lane executing).  The bank of byte a is (a / 4) % 64 for both, so an image is free of conflicts when the 16-byte
// slots (32-byte chunks) that one lane group reads are distinct modulo the 256-byte bank row.  The groups: ds_read_b128 serves lanes
// {0-3, 12-15, 20-27} together (likewise the other three quarters), which are rows {0-3, 12-15} at slot c and rows {4-11} at slot c ^ 1;
// ds_read_b64_tr_b16 serves lanes 0-31, which are 8 consecutive rows (from a multiple of 8) at one chunk.
//   DP = 96   192-byte rows of 12 slots / 6 chunks.  A row starts at slot 12 row % 16 = 4 (-row & 3): the rows of an aligned quad differ
//             in the upper two slot bits already.  Only bits that stay inside the row may be swizzled: the lower two slot bits ^=
//             -(row >> 2) & 3 (quads 0..3 of a 16-row block get 0, 3, 2, 1, so a group's quads read lower bits c, (c ^ 1) ^ 3, (c ^ 1) ^ 2,
//             c ^ 1: four different values); the lowest chunk bit ^= (row >> 2) & 1 (the two quads of 8 rows)
//   DP = 128  256-byte rows = one bank row each: slot ^= row & 15, chunk ^= row & 7
template <int DP>
__device__ __forceinline__ int lk_off(int row, int c) {
    static_assert(DP == 96 || DP == 128, "padded head dim");
    if constexpr (DP == 96) return row * 192 + ((c ^ (-(row >> 2) & 3)) << 4);
    else return row * 256 + ((c ^ (row & 15)) << 4);
}
template <int DP>
__device__ __forceinline__ int lt_off(int row, int d) {
    static_assert(DP == 96 || DP == 128, "padded head dim");
    if constexpr (DP == 96) return row * 192 + ((((d >> 4) ^ ((row >> 2) & 1))) << 5) + ((d & 15) << 1);
    else return row * 256 + ((((d >> 4) ^ (row & 7))) << 5) + ((d & 15) << 1);
}

// operand fragment of 16 rows (rowblk) x 32 columns (k step ks): lane holds row 16 rowblk + (lane & 15), columns 32 ks + 8 (lane >> 4) + 0..7
template <int DP>
__device__ __forceinline__ bf16x8 l_frag_rows(const char* tile, int rowblk, int ks, int lane) {
    const int row = rowblk * 16 + (lane & 15);
    return *reinterpret_cast<const bf16x8*>(tile + lk_off<DP>(row, 4 * ks + (lane >> 4)));
}
// transposed operand [i = d (16, block dt)][k = 8 rows]: rows rowa + 4g + 0..3 and rowb + 4g + 0..3 — the k order of a packed pair of
// accumulator tiles (rows 4g + r of tile a, then of tile b).  Every lane of the wave must execute it (cross-lane gather).
template <int DP>
__device__ __forceinline__ bf16x8 l_frag_tr(const char* tile, int rowa, int rowb, int dt, int lane) {
    const int i = lane & 15, g = lane >> 4;
    const int ra = rowa + 4 * g + (i >> 2), rb = rowb + 4 * g + (i >> 2);
    const int col = 16 * dt + 4 * (i & 3);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_l*)(tile + lt_off<DP>(ra, col)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_l*)(tile + lt_off<DP>(rb, col)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}
// 16 rows of a [T][D] bf16 matrix (row pitch `pitch`) as an MFMA operand straight from global memory: the lane passes its own row q
// (first row + (lane & 15)) and receives columns 32 ks + 8 (lane >> 4) + 0..7 (zeros past T and from column D on)
template <int DP>
__device__ __forceinline__ void l_load_rows(const bf16_t* __restrict__ base, int64_t pitch, int q, int T, int g, bf16x8 (&f)[DP / 32], int D) {
#pragma unroll
    for (int ks = 0; ks < DP / 32; ++ks) {
        uint4 u = make_uint4(0, 0, 0, 0);
        if (q < T && 32 * ks + 8 * g < D) u = *reinterpret_cast<const uint4*>(base + (int64_t)q * pitch + 32 * ks + 8 * g);
        f[ks] = __builtin_bit_cast(bf16x8, u);
    }
}

// K / V block staging for the forward and dQ kernels: 64 keys x DP / 8 16-byte chunks of K and of V = DP / 32 + DP / 32 vectors per thread
// (256 threads), zeros for keys past T (their scores are masked; a zero V row keeps 0 x garbage out of the P V product) and for chunks
// from column D on
template <int DP>
struct KVRegsT { uint4 k[DP / 32], v[DP / 32]; };
template <int DP>
__device__ __forceinline__ void kv_fetch(KVRegsT<DP>& r, const bf16_t* __restrict__ base, int64_t pitch, int E, int key0, int T, int D) {
#pragma unroll
    for (int it = 0; it < DP / 32; ++it) {
        const int idx = threadIdx.x + 256 * it, key = key0 + idx / (DP / 8), c = idx % (DP / 8);
        r.k[it] = make_uint4(0, 0, 0, 0); r.v[it] = make_uint4(0, 0, 0, 0);
        if (key < T && 8 * c < D) {
            r.k[it] = *reinterpret_cast<const uint4*>(base + (int64_t)key * pitch + E + 8 * c);
            r.v[it] = *reinterpret_cast<const uint4*>(base + (int64_t)key * pitch + 2 * E + 8 * c);
        }
    }
}
// Kr: K row image, Kt: K tr image (nullptr = not wanted), Vr: V row image (nullptr = not wanted), Vt: V tr image (nullptr = not wanted)
template <int DP>
__device__ __forceinline__ void kv_store(const KVRegsT<DP>& r, char* Kr, char* Kt, char* Vr, char* Vt) {
#pragma unroll
    for (int it = 0; it < DP / 32; ++it) {
        const int idx = threadIdx.x + 256 * it, key = idx / (DP / 8), c = idx % (DP / 8);
        *reinterpret_cast<uint4*>(Kr + lk_off<DP>(key, c)) = r.k[it];
        if (Kt) *reinterpret_cast<uint4*>(Kt + lt_off<DP>(key, 8 * c)) = r.k[it];
        if (Vr) *reinterpret_cast<uint4*>(Vr + lk_off<DP>(key, c)) = r.v[it];
        if (Vt) *reinterpret_cast<uint4*>(Vt + lt_off<DP>(key, 8 * c)) = r.v[it];
    }
}

// Query tile staging for the dK / dV kernels, 32 rows per step: Q rows, Q tr, dO rows, dO tr images (32 rows x 2 DP bytes = QT_IMG<DP> each: 6 or
// 8 KiB), then lse (x log2 e) and delta of the 32 rows.
template <int DP> constexpr int QT_IMG = 32 * 2 * DP;
template <int DP> constexpr int QT_BYTES_DP = 4 * QT_IMG<DP> + 2 * 32 * 4;
template <int DP> constexpr int QT_ITERS = (32 * (DP / 8) + 255) / 256;      // 2 (DP = 96: the second by half of the threads)

template <int DP>
struct QRegsT { uint4 q[QT_ITERS<DP>], o[QT_ITERS<DP>]; float ls[QT_ITERS<DP>], dl[QT_ITERS<DP>]; };
// vector i = thread + 256 it: query row i / (DP / 8) of the tile, 16-byte chunk i % (DP / 8) (32 rows x DP / 8 chunks); rows past T: zeros,
// lse = +huge (P = 0); chunks from column D on: zeros
template <int DP>
__device__ __forceinline__ void qt_fetch(QRegsT<DP>& r, const bf16_t* __restrict__ base, int64_t pitch, const bf16_t* __restrict__ dob, int E,
                                         const float* __restrict__ lse_bh, const float* __restrict__ del_bh, int q0, int T, int D) {
#pragma unroll
    for (int it = 0; it < QT_ITERS<DP>; ++it) {
        const unsigned idx = threadIdx.x + 256 * it;
        const int row = idx / (DP / 8), c = idx % (DP / 8), q = q0 + row;
        r.q[it] = make_uint4(0, 0, 0, 0); r.o[it] = make_uint4(0, 0, 0, 0); r.ls[it] = 1e30f; r.dl[it] = 0.f;
        if (q < T && row < 32 && 8 * c < D) {
            r.q[it] = *reinterpret_cast<const uint4*>(base + (int64_t)q * pitch + 8 * c);
            r.o[it] = *reinterpret_cast<const uint4*>(dob + (int64_t)q * E + 8 * c);
            if (c == 0) { r.ls[it] = lse_bh[q] * LOG2E; r.dl[it] = del_bh[q]; }
        }
    }
}
template <int DP>
__device__ __forceinline__ void qt_store(const QRegsT<DP>& r, char* tile) {
#pragma unroll
    for (int it = 0; it < QT_ITERS<DP>; ++it) {
        const unsigned idx = threadIdx.x + 256 * it;
        const int row = idx / (DP / 8), c = idx % (DP / 8);
        if (row < 32) {
            *reinterpret_cast<uint4*>(tile + lk_off<DP>(row, c)) = r.q[it];
            *reinterpret_cast<uint4*>(tile + QT_IMG<DP> + lt_off<DP>(row, 8 * c)) = r.q[it];
            *reinterpret_cast<uint4*>(tile + 2 * QT_IMG<DP> + lk_off<DP>(row, c)) = r.o[it];
            *reinterpret_cast<uint4*>(tile + 3 * QT_IMG<DP> + lt_off<DP>(row, 8 * c)) = r.o[it];
            if (c == 0) {
                float* ld = reinterpret_cast<float*>(tile + 4 * QT_IMG<DP>);
                ld[row] = r.ls[it]; ld[32 + row] = r.dl[it];
            }
        }
    }
}

// =====================================================================================================================================
// Forward
// =====================================================================================================================================
template <bool DROP, Rows L, int DP>
__device__ __forceinline__ void attn_stream_fwd_body(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, float* __restrict__ lse,
                                                     const int* __restrict__ lens, int T, int H, int nqb, int B, int Mq, float scale,
                                                     float drop_p, uint32_t drop_seed, int D) {
    constexpr bool PACKED = L == Rows::Packed;
    constexpr int KS = DP / 32, DT = DP / 16;      // k steps of Q K^T, 16-column tiles of O
    __shared__ __attribute__((aligned(16))) char smem[2][2][LKB * 2 * DP];      // [buffer][K rows, V tr][64 keys x 2 DP B]
    const bool last_dt = D > 16 * (DT - 1);      // O's last tile holds a column below D (uniform)
    const int E = H * D;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const UttRows<L> utt(lens, b, T, Mq);
    const int Tb = utt.Tb;      // one value per workgroup: everything that depends on it is workgroup-uniform
    const bf16_t* base = qkv + utt.r0 * pitch + h * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int q = qblk * LQB + 16 * wave + lc;
    bf16_t* dst = ctx + (utt.r0 + q) * E + h * D + 4 * g;
    float* lse_q = lse + ((int64_t)b * H + h) * T + q;
    if constexpr (PACKED) zero_tail_vectors(reinterpret_cast<uint4*>(ctx), lens, B, Mq, E / 8);
    if constexpr (L != Rows::Fixed) {
        if (qblk * LQB >= Tb) {      // the whole query block is padding: zeros, and out before any barrier (uniform: qblk and Tb are)
            if (q < T) {
                if (g == 0) *lse_q = 0.f;      // lse is padded in every layout
                if constexpr (!PACKED) {       // packed: these rows are another utterance's
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        if (16 * dt + 4 * g < D) *reinterpret_cast<uint2*>(dst + 16 * dt) = make_uint2(0u, 0u);
                }
            }
            return;
        }
    }
    const int nkb = (Tb + LKB - 1) / LKB;
    bf16x8 qf[KS];
    l_load_rows<DP>(base, pitch, q, Tb, g, qf, D);
    KVRegsT<DP> r;
    kv_fetch(r, base, pitch, E, 0, Tb, D);
    kv_store(r, smem[0][0], nullptr, nullptr, smem[0][1]);
    __syncthreads();
    const float sl2 = scale * LOG2E;
    const uint64_t rowbase = (((uint64_t)b * H + h) * T + (uint64_t)(q < T ? q : 0)) * (uint64_t)T;      // mask index: the padded T
    float m = -INFINITY, l = 0.f;      // running max (raw score units) and this lane's share of the running sum
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
        const int p = kb & 1;
        if (kb + 1 < nkb) kv_fetch(r, base, pitch, E, (kb + 1) * LKB, Tb, D);      // in flight under this block's products
        const char* Kr = smem[p][0];
        const char* Vt = smem[p][1];
        const int key0 = kb * LKB;
        f32x4 s[4];
        float mb = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_rows<DP>(Kr, t, ks, lane), qf[ks], s[t], 0, 0, 0);
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
        for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
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
            for (int dt = 0; dt < DT; ++dt)
                if (dt < DT - 1 || last_dt)      // a tile of zero columns needs no product
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_tr<DP>(Vt, 32 * u, 32 * u + 16, dt, lane), pf, o[dt], 0, 0, 0);
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
            for (int dt = 0; dt < DT; ++dt)
                if (16 * dt + 4 * g < D)      // columns from D on are the next head's
                    *reinterpret_cast<uint2*>(dst + 16 * dt) = valid ? make_uint2(pack_bf2(o[dt][0] * inv, o[dt][1] * inv), pack_bf2(o[dt][2] * inv, o[dt][3] * inv))
                                                                     : make_uint2(0u, 0u);
        }
    }
}

// =====================================================================================================================================
// Backward
// =====================================================================================================================================
// delta[(b*H + h)*T + q] = <dO, O> of the row for q < Tb, 0 beyond (those rows of ctx / dctx are not read); one thread group of 8 per
// (b, q, h) of the PADDED space in every layout, rows = B * T * H.  A row is D / 8 16-byte pieces: lane c of the 8 sums piece c, then piece
// c + 8 where 8 (c + 8) < D, then the 8 lanes are summed — a fixed order
template <Rows L>
__device__ __forceinline__ void attn_stream_delta_body(const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx, float* __restrict__ delta,
                                                       const int* __restrict__ lens, int64_t rows, int T, int H, int Mq, int D) {
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
#pragma unroll
            for (int i = 0; i < 2; ++i) {      // D <= 128: at most 16 pieces
                const int pc = c + 8 * i;
                if (8 * pc < D) {
                    const uint4 vo = *reinterpret_cast<const uint4*>(dctx + src * D + 8 * pc);
                    const uint4 vc = *reinterpret_cast<const uint4*>(ctx + src * D + 8 * pc);
                    const unsigned ow[4] = {vo.x, vo.y, vo.z, vo.w}, cw[4] = {vc.x, vc.y, vc.z, vc.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        dot += __uint_as_float(ow[k] << 16) * __uint_as_float(cw[k] << 16);
                        dot += __uint_as_float(ow[k] & 0xFFFF0000u) * __uint_as_float(cw[k] & 0xFFFF0000u);
                    }
                }
            }
        }
    }
    dot = lanes8_sum(dot);
    if (row < rows && c == 0) delta[(b * H + h) * T + q] = dot;
}

// ---- dK / dV ------------------------------------------------------------------------------------------------------------------------
// Query tiles of 32 rows per step: QRegsT / qt_fetch / qt_store (Q rows, Q tr, dO rows, dO tr images, lse x log2 e, delta).  All three layouts,
// the fixed one included (attention_long.hip's hand-written dK / dV kernel is for head dim 64)
template <bool DROP, Rows L, int DP>
__device__ __forceinline__ void attn_stream_dkdv_body(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      bf16_t* __restrict__ dqkv, const int* __restrict__ lens, int T, int H, int nkw, int Mq,
                                                      float scale, float drop_p, uint32_t drop_seed, int D) {
    constexpr bool PACKED = L == Rows::Packed;
    constexpr int KS = DP / 32, DT = DP / 16;
    __shared__ __attribute__((aligned(16))) char smem[2][QT_BYTES_DP<DP>];
    const bool last_dt = D > 16 * (DT - 1);
    const int E = H * D;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nkw, kblk = blockIdx.x % nkw;
    const int b = bh / H, h = bh % H;
    const UttRows<L> utt(lens, b, T, Mq);
    const int Tb = utt.Tb;      // one value per workgroup
    const bf16_t* base = qkv + utt.r0 * pitch + h * D;
    const bf16_t* dob = dctx + utt.r0 * E + h * D;
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
                bf16_t* dst = dqkv + (utt.r0 + key) * pitch + h * D + 4 * g;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    if (16 * dt + 4 * g < D) {
                        *reinterpret_cast<uint2*>(dst + E + 16 * dt) = make_uint2(0u, 0u);
                        *reinterpret_cast<uint2*>(dst + 2 * E + 16 * dt) = make_uint2(0u, 0u);
                    }
            }
        }
        return;
    }
    // the wave's K / V rows as B operands (lane: key key_w + 16 j + lc, d = 32 ks + 8 g + 0..7)
    bf16x8 kf[2][KS], vf[2][KS];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        l_load_rows<DP>(base + E, pitch, key_w + 16 * j + lc, Tb, g, kf[j], D);
        l_load_rows<DP>(base + 2 * E, pitch, key_w + 16 * j + lc, Tb, g, vf[j], D);
    }
    const int nqt = (Tb + 31) / 32;
    QRegsT<DP> r;
    qt_fetch(r, base, pitch, dob, E, lse_bh, del_bh, 0, Tb, D);
    qt_store(r, smem[0]);
    __syncthreads();
    f32x4 dVt[DT][2], dKt[DT][2];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { dVt[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; dKt[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const float sc2 = scale * LOG2E;
    for (int u = 0; u < nqt; ++u) {
        const int p = u & 1;
        if (u + 1 < nqt) qt_fetch(r, base, pitch, dob, E, lse_bh, del_bh, 32 * (u + 1), Tb, D);
        const char* Qk = smem[p];
        const char* Qt = Qk + QT_IMG<DP>;
        const char* Ok = Qk + 2 * QT_IMG<DP>;
        const char* Ot = Qk + 3 * QT_IMG<DP>;
        const float* lsP = reinterpret_cast<const float*>(Qk + 4 * QT_IMG<DP>);
        const float* dlP = lsP + 32;
        float lq[2][4], dq_[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float4 l4 = *reinterpret_cast<const float4*>(lsP + 16 * a + 4 * g), d4 = *reinterpret_cast<const float4*>(dlP + 16 * a + 4 * g);
            lq[a][0] = l4.x; lq[a][1] = l4.y; lq[a][2] = l4.z; lq[a][3] = l4.w;
            dq_[a][0] = d4.x; dq_[a][1] = d4.y; dq_[a][2] = d4.z; dq_[a][3] = d4.w;
        }
        f32x4 P[2][2], dS[2][2];      // [query tile a][key tile j]: D[q = 16a + 4g + r][key = 16j + lc]
        // query tile a outside and its Q / dO fragments loaded per tile (the 64 body holds both tiles' fragments with key tile j outside):
        // with 8 DP / 8 accumulator and DP / 2 K / V fragment registers, that is what keeps DP = 128 with dropout free of spills
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            bf16x8 qa[KS], oa[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { qa[ks] = l_frag_rows<DP>(Qk, a, ks, lane); oa[ks] = l_frag_rows<DP>(Ok, a, ks, lane); }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int key = key_w + 16 * j + lc;
                f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], kf[j][ks], sv, 0, 0, 0);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa[ks], vf[j][ks], dp, 0, 0, 0);
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
        for (int dt = 0; dt < DT; ++dt) {
            if (dt < DT - 1 || last_dt) {      // a tile of zero columns needs no product
                const bf16x8 ot = l_frag_tr<DP>(Ot, 0, 16, dt, lane);
                const bf16x8 qt = l_frag_tr<DP>(Qt, 0, 16, dt, lane);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    dVt[dt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ot, pP[j], dVt[dt][j], 0, 0, 0);
                    dKt[dt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, pS[j], dKt[dt][j], 0, 0, 0);
                }
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
            bf16_t* dst = dqkv + (utt.r0 + key) * pitch + h * D + 4 * g;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (16 * dt + 4 * g >= D) continue;      // columns from D on are the next head's
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
template <bool DROP, Rows L, int DP>
__device__ __forceinline__ void attn_stream_dq_body(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dctx,
                                                    const float* __restrict__ lse, const float* __restrict__ delta,
                                                    bf16_t* __restrict__ dqkv, const int* __restrict__ lens, int T, int H, int nqb, int B, int Mq,
                                                    float scale, float drop_p, uint32_t drop_seed, int D) {
    constexpr bool PACKED = L == Rows::Packed;
    constexpr int KS = DP / 32, DT = DP / 16;
    __shared__ __attribute__((aligned(16))) char smem[2][3][LKB * 2 * DP];      // [buffer][K rows, K tr, V rows]
    const bool last_dt = D > 16 * (DT - 1);
    const int E = H * D;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const UttRows<L> utt(lens, b, T, Mq);
    const int Tb = utt.Tb;      // one value per workgroup
    const bf16_t* base = qkv + utt.r0 * pitch + h * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int q0 = qblk * LQB + 16 * wave, q = q0 + lc;
    bf16_t* dst = dqkv + (utt.r0 + q) * pitch + h * D + 4 * g;
    if constexpr (PACKED) zero_tail_vectors(reinterpret_cast<uint4*>(dqkv), lens, B, Mq, 3 * E / 8);
    if constexpr (L != Rows::Fixed) {
        if (qblk * LQB >= Tb) {      // the whole query block is padding: zero dQ rows, and out before any barrier (uniform: qblk and Tb are)
            if constexpr (PACKED) return;      // packed: these rows are another utterance's
            if (q < T) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    if (16 * dt + 4 * g < D) *reinterpret_cast<uint2*>(dst + 16 * dt) = make_uint2(0u, 0u);
            }
            return;
        }
    }
    const int nkb = (Tb + LKB - 1) / LKB;
    bf16x8 qf[KS], of[KS];
    l_load_rows<DP>(base, pitch, q, Tb, g, qf, D);
    l_load_rows<DP>(dctx + utt.r0 * E + h * D, E, q, Tb, g, of, D);
    const int64_t rbh = ((int64_t)b * H + h) * T;
    const float lq = q < Tb ? lse[rbh + q] * LOG2E : 1e30f;
    const float dl = q < Tb ? delta[rbh + q] : 0.f;
    KVRegsT<DP> r;
    kv_fetch(r, base, pitch, E, 0, Tb, D);
    kv_store(r, smem[0][0], smem[0][1], smem[0][2], nullptr);
    __syncthreads();
    const float sc2 = scale * LOG2E;
    const uint64_t rowbase = ((uint64_t)rbh + (uint64_t)(q < T ? q : 0)) * (uint64_t)T;      // mask index: the padded T
    f32x4 dq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
        const int p = kb & 1;
        if (kb + 1 < nkb) kv_fetch(r, base, pitch, E, (kb + 1) * LKB, Tb, D);
        const char* Kr = smem[p][0];
        const char* Kt = smem[p][1];
        const char* Vr = smem[p][2];
        const int key0 = kb * LKB;
        f32x4 ds[4];      // dS^T[key = 16t + 4g + r][q = lc]
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_rows<DP>(Kr, t, ks, lane), qf[ks], sv, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_rows<DP>(Vr, t, ks, lane), of[ks], dp, 0, 0, 0);
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
            for (int dt = 0; dt < DT; ++dt)
                if (dt < DT - 1 || last_dt)      // a tile of zero columns needs no product
                    dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_tr<DP>(Kt, 32 * u, 32 * u + 16, dt, lane), sf, dq[dt], 0, 0, 0);
        }
        if (kb + 1 < nkb) kv_store(r, smem[p ^ 1][0], smem[p ^ 1][1], smem[p ^ 1][2], nullptr);
        __syncthreads();
    }
    if (q < (PACKED ? Tb : T)) {      // packed: nothing is stored at or beyond Tb
        const bool valid = q < Tb;      // padded query rows of the last valid block: zeros, as the blocks beyond it
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            if (16 * dt + 4 * g < D)      // columns from D on are the next head's
                *reinterpret_cast<uint2*>(dst + 16 * dt) = valid ? make_uint2(pack_bf2(dq[dt][0] * scale, dq[dt][1] * scale), pack_bf2(dq[dt][2] * scale, dq[dt][3] * scale))
                                                                 : make_uint2(0u, 0u);
    }
}

}  // namespace wide
}  // namespace
