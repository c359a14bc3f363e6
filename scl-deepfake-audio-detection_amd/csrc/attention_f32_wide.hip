// attention_f32_wide.hip — the fp32 streaming attention over packed valid frames (attention_f32.hip) for head dims 72..128 (D % 8 == 0), on a
// PADDED head dim DP: DP = 96 serves D = 72..96, DP = 128 serves D = 104..128 (XLS-R 1B: 80, 2B: 120), as attention_wide.hip /
// attn_wide_body.h do for the bf16 bodies.  scl_attn_fwd_packed_f32 (attention_f32.hip) validates its arguments and hands a head dim that
// scl_attn_wide_takes over to scl_attn_wide_fwd_f32 here; the 64-wide kernel stays in its own file, textually apart.
//
//   qkv f32 [Mq, 3, H, D] -> ctx f32 [Mq, H*D]; utterance b owns rows row0[b] .. row0[b + 1] - 1 (UttRows<Rows::Packed>).  Forward only: no
//   lse, no dropout.
//
// THE TILE SCHEME AND THE ARITHMETIC are attention_f32.hip's: one workgroup per (utterance, head, 64 queries), four waves of 16 queries;
// keys stream through LDS in blocks of KB, double-buffered, the next block's global loads in flight under the current block's products;
// every f32 operand x is hi = bf16(x), lo = bf16(x - hi) (Q split when its rows are loaded, K / V between the global load and the LDS
// write, P in registers) and a product is lo hi + hi lo + hi hi, small terms first, on v_mfma_f32_16x16x32_bf16 into ONE f32 accumulator
// per tile; online soft-max in fp32 with the rescale on every block; every output element is summed by one wave in a fixed order (no
// atomics: the same bits on every run, and the bits an utterance gets alone).
//
// THE PADDING is attn_wide_body.h's, for f32 rows.  In memory a head is D floats wide; columns D..DP-1 of a head's row are the next
// head's data (the next section's, or lie past the buffer) and are never read or written.  An 8-float chunk c of a q / k / v row is
// loaded when 8 c < D and is zero in registers and LDS otherwise; a 4-column output group 16 dt + 4 g is stored when it lies below D;
// the last 16-column tile of O gets no MFMA when it lies at or beyond D (D <= 80 at DP = 96, D <= 112 at DP = 128: workgroup-uniform).
// D % 8 == 0 keeps every float4 load and store 16-byte aligned at h * D.
//
// THE STORES are attention_f32.hip's: no row at or beyond an utterance's end is loaded or stored, a query block that starts at or
// beyond Tb leaves before its first barrier, rows [row0[B], Mq) of ctx are written as zeros by every launch, rows >= Mq are never touched.
//
// THE TILE BUDGET.  Four images per key block (K hi / lo as rows, V hi / lo transposed; lk_off / lt_off of attn_wide_body.h, rows of
// 2 DP bytes), double-buffered: LDS = 2 x 4 x KB x 2 DP bytes.
//   KB = 64 (the 64-wide kernel's block)   96 KiB at DP = 96, 128 KiB at DP = 128: one workgroup (4 waves) per CU, DP / 8 float4 of f32
//                                          staging per thread
//   KB = 32                                48 / 64 KiB: two workgroups per CU (__launch_bounds__(256, 2): at most 256 registers), 8 float4
//                                          of staging (two rounds of the 256 threads), twice the rescales and barriers per key
// THE CHOICE is KB = 32, by measurement (profiles/score_pack_headdim.txt): both builds timed side by side per layer at
// batch 64 x 16 heads, KB = 32 takes 0.53 - 0.61 of KB = 64's time (D = 80: 118 against 220 us at 201 frames, 188 against 349 us on the
// ragged 624-frame batch; D = 120: 189 against 322, 286 against 475).  With one wave per SIMD nothing covers the LDS read latency in
// front of each group of three dependent MFMAs, the soft-max and the split / LDS-store phase between blocks; a second workgroup on the
// CU does.  SCL_ATTN_F32_WIDE_KB=64 (SCL_BUILD_DEFINES) builds the other variant for such a comparison.
#include "attn_wide_body.h"
#include "attn_wide.h"

#ifndef SCL_ATTN_F32_WIDE_KB
#define SCL_ATTN_F32_WIDE_KB 32
#endif

namespace {

typedef __attribute__((ext_vector_type(8))) float f32x8a;

// eight f32 (two 16-byte vectors) -> the hi and lo bf16 planes, 16 bytes each (split8 of attention_f32.hip)
__device__ __forceinline__ void split8(const float4& a, const float4& b, uint4& hi, uint4& lo) {
    const f32x8a x = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const bf16x8 h = __builtin_convertvector(x, bf16x8);
    const f32x8a back = __builtin_convertvector(h, f32x8a);
    const bf16x8 l = __builtin_convertvector(x - back, bf16x8);
    hi = __builtin_bit_cast(uint4, h);
    lo = __builtin_bit_cast(uint4, l);
}

// the lane's query row as the B operand of every k step, hi and lo planes (columns 32 ks + 8 g + 0..7; zeros past Tb and from column D on)
template <int DP>
__device__ __forceinline__ void q_load_split(const float* __restrict__ base, int64_t pitch, int q, int Tb, int g, bf16x8 (&qh)[DP / 32],
                                             bf16x8 (&ql)[DP / 32], int D) {
#pragma unroll
    for (int ks = 0; ks < DP / 32; ++ks) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (q < Tb && 32 * ks + 8 * g < D) {
            const float4* src = reinterpret_cast<const float4*>(base + (int64_t)q * pitch + 32 * ks + 8 * g);
            a = src[0]; b = src[1];
        }
        uint4 h, l;
        split8(a, b, h, l);
        qh[ks] = __builtin_bit_cast(bf16x8, h);
        ql[ks] = __builtin_bit_cast(bf16x8, l);
    }
}

// K / V block staging in f32: KB keys x DP / 8 chunks of 8 floats of K and of V over 256 threads (wide::kv_fetch's thread / chunk map: vector
// idx = thread + 256 it is key idx / (DP / 8), chunk idx % (DP / 8)); zeros for keys past Tb (their scores are masked; a zero V row keeps
// 0 x garbage out of the P V product) and for chunks from column D on.  KB = 32 at DP = 96 is 384 vectors: the second round by half of
// the threads (PARTIAL).
template <int DP, int KB>
struct KVRegsF {
    static constexpr int VECS = KB * (DP / 8);
    static constexpr int ITERS = (VECS + 255) / 256;
    static constexpr bool PARTIAL = VECS % 256 != 0;
    float4 k[ITERS][2], v[ITERS][2];
};
template <int DP, int KB>
__device__ __forceinline__ void kvf_fetch(KVRegsF<DP, KB>& r, const float* __restrict__ base, int64_t pitch, int E, int key0, int Tb, int D) {
#pragma unroll
    for (int it = 0; it < KVRegsF<DP, KB>::ITERS; ++it) {
        const int idx = threadIdx.x + 256 * it, kin = idx / (DP / 8), key = key0 + kin, c = idx % (DP / 8);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        r.k[it][0] = z; r.k[it][1] = z; r.v[it][0] = z; r.v[it][1] = z;
        if ((!KVRegsF<DP, KB>::PARTIAL || kin < KB) && key < Tb && 8 * c < D) {
            const float4* ks = reinterpret_cast<const float4*>(base + (int64_t)key * pitch + E + 8 * c);
            const float4* vs = reinterpret_cast<const float4*>(base + (int64_t)key * pitch + 2 * E + 8 * c);
            r.k[it][0] = ks[0]; r.k[it][1] = ks[1];
            r.v[it][0] = vs[0]; r.v[it][1] = vs[1];
        }
    }
}
// buf: [K hi rows | K lo rows | V hi tr | V lo tr], KB * 2 DP bytes each
template <int DP, int KB>
__device__ __forceinline__ void kvf_store(const KVRegsF<DP, KB>& r, char* buf) {
    constexpr int IMG = KB * 2 * DP;
#pragma unroll
    for (int it = 0; it < KVRegsF<DP, KB>::ITERS; ++it) {
        const int idx = threadIdx.x + 256 * it, kin = idx / (DP / 8), c = idx % (DP / 8);
        uint4 kh, kl, vh, vl;
        split8(r.k[it][0], r.k[it][1], kh, kl);
        split8(r.v[it][0], r.v[it][1], vh, vl);
        if (!KVRegsF<DP, KB>::PARTIAL || kin < KB) {
            *reinterpret_cast<uint4*>(buf + wide::lk_off<DP>(kin, c)) = kh;
            *reinterpret_cast<uint4*>(buf + IMG + wide::lk_off<DP>(kin, c)) = kl;
            *reinterpret_cast<uint4*>(buf + 2 * IMG + wide::lt_off<DP>(kin, 8 * c)) = vh;
            *reinterpret_cast<uint4*>(buf + 3 * IMG + wide::lt_off<DP>(kin, 8 * c)) = vl;
        }
    }
}

template <int DP, int KB>
constexpr int f32_wide_lds = 2 * 4 * KB * 2 * DP;
// two workgroups per CU where the CU's 160 KiB of LDS hold them
template <int DP, int KB>
constexpr int f32_wide_wgs = 2 * f32_wide_lds<DP, KB> <= 160 * 1024 ? 2 : 1;

template <int DP, int KB>
__global__ __launch_bounds__(256, (f32_wide_wgs<DP, KB>)) void attn_fwd_packed_f32_wide_kernel(const float* __restrict__ qkv, float* __restrict__ ctx,
                                                                                              const int* __restrict__ row0, int T, int H, int D,
                                                                                              int nqb, int B, int Mq, float scale) {
    static_assert(KB == 32 || KB == 64, "keys per block");
    constexpr int KS = DP / 32, DT = DP / 16;      // k steps of Q K^T, 16-column tiles of O
    constexpr int NT = KB / 16, NU = KB / 32;      // 16-key score tiles, 32-key steps of P V
    constexpr int IMG = KB * 2 * DP;
    __shared__ __attribute__((aligned(16))) char smem[2][4 * IMG];      // [buffer][K hi rows, K lo rows, V hi tr, V lo tr]
    const bool last_dt = D > 16 * (DT - 1);      // O's last tile holds a column below D (uniform)
    const int E = H * D;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const UttRows<Rows::Packed> utt(row0, b, T, Mq);
    const int Tb = utt.Tb;      // one value per workgroup: everything that depends on it is workgroup-uniform
    const float* base = qkv + utt.r0 * pitch + h * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int q = qblk * LQB + 16 * wave + lc;
    zero_tail_vectors(reinterpret_cast<uint4*>(ctx), row0, B, Mq, E / 4);
    if (qblk * LQB >= Tb) return;      // these rows are another utterance's (or nobody's): out before any barrier, no store (uniform)
    const int nkb = (Tb + KB - 1) / KB;
    bf16x8 qh[KS], ql[KS];
    q_load_split<DP>(base, pitch, q, Tb, g, qh, ql, D);
    KVRegsF<DP, KB> r;
    kvf_fetch(r, base, pitch, E, 0, Tb, D);
    kvf_store(r, smem[0]);
    __syncthreads();
    const float sl2 = scale * LOG2E;
    float m = -INFINITY, l = 0.f;      // running max (raw score units) and this lane's share of the running sum
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
        const int p = kb & 1;
        if (kb + 1 < nkb) kvf_fetch(r, base, pitch, E, (kb + 1) * KB, Tb, D);      // in flight under this block's products
        const char* Kh = smem[p];
        const char* Kl = Kh + IMG;
        const char* Vh = Kh + 2 * IMG;
        const char* Vl = Kh + 3 * IMG;
        const int key0 = kb * KB;
        f32x4 s[NT];
        float mb = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {      // small terms first, then hi hi
                const bf16x8 kh = wide::l_frag_rows<DP>(Kh, t, ks, lane);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wide::l_frag_rows<DP>(Kl, t, ks, lane), qh[ks], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql[ks], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh[ks], s[t], 0, 0, 0);
            }
            if (key0 + KB > Tb) {      // the last block only
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
        f32x4 sl[NT];      // p - bf16(p)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][rr], sl2, msl));
                ls += pv;
                s[t][rr] = pv;
                sl[t][rr] = pv - bf2f(f2bf(pv));
            }
        l = l * alpha + ls;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const bf16x8 ph = l_pack8(s[2 * u], s[2 * u + 1]);
            const bf16x8 pl = l_pack8(sl[2 * u], sl[2 * u + 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (dt < DT - 1 || last_dt) {      // a tile of zero columns needs no product
                    const bf16x8 vh = wide::l_frag_tr<DP>(Vh, 32 * u, 32 * u + 16, dt, lane);
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wide::l_frag_tr<DP>(Vl, 32 * u, 32 * u + 16, dt, lane), ph, o[dt], 0, 0, 0);
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pl, o[dt], 0, 0, 0);
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, ph, o[dt], 0, 0, 0);
                }
            }
        }
        if (kb + 1 < nkb) kvf_store(r, smem[p ^ 1]);      // its last readers finished before the previous barrier
        __syncthreads();
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    if (q < Tb) {      // nothing is stored at or beyond Tb
        float* dst = ctx + (utt.r0 + q) * E + h * D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            if (16 * dt + 4 * g < D)      // columns from D on are the next head's
                *reinterpret_cast<float4*>(dst + 16 * dt) = make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    }
}

template <int DP>
void launch(const float* qkv, float* ctx, const int32_t* row0, int B, int T, int H, int D, int Mq, float scale, hipStream_t s) {
    const int nqb = (T + LQB - 1) / LQB;
    hipLaunchKernelGGL((attn_fwd_packed_f32_wide_kernel<DP, SCL_ATTN_F32_WIDE_KB>), dim3((unsigned)(B * H * nqb)), dim3(256), 0, s, qkv, ctx,
                       (const int*)row0, T, H, D, nqb, B, Mq, scale);
}

}  // namespace

// the arguments of scl_attn_fwd_packed_f32, which has validated the row counts, the pointers and the grid
int scl_attn_wide_fwd_f32(const float* qkv, float* ctx, const int32_t* row0, int B, int T, int H, int D, int Mq, float scale, void* stream) {
    SCL_REQUIRE(scl_attn_wide_takes(D), "attn_fwd_packed_f32: " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);
    if (D <= 96) launch<96>(qkv, ctx, row0, B, T, H, D, Mq, scale, (hipStream_t)stream);
    else launch<128>(qkv, ctx, row0, B, T, H, D, Mq, scale, (hipStream_t)stream);
    return scl_check_launch("scl_attn_fwd_packed_f32");
}
