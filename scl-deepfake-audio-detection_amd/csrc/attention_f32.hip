// attention_f32.hip — streaming attention with fp32 accuracy over packed valid frames: the scoring path's attention (Encoder.forward_f32
// with packed=(row0, Mq)) without a T x T score buffer and without the padded rows.
//
//   scl_attn_fwd_packed_f32   qkv f32 [Mq, 3, H, 64] -> ctx f32 [Mq, H*64] (head dims 72..128 in steps of 8: the entry hands them to
//                             attention_f32_wide.hip, the same scheme on a padded head dim); utterance b owns rows row0[b] .. row0[b + 1] - 1 (row0 int32
//                             [B + 1] on the device, the layout of attention_packed.hip: Tb and the first row are clamped as UttRows<Rows::Packed>
//                             does, Mv = row0[B] is read on the device).  Forward only: no lse, no dropout.
//
// THE TILE SCHEME is attn_stream_fwd_body's (attn_stream_body.h): one workgroup per (utterance, head, 64 queries), four waves of 16
// queries; keys stream through LDS in blocks of 64, double-buffered, the next block's global loads in flight under the current block's
// products; S^T = K Q^T so that a lane holds one query's scores, online soft-max in fp32 with the rescale on every block; every output
// element is summed by one wave in a fixed order (no atomics: the same bits on every run, and the bits an utterance gets alone).
//
// THE ARITHMETIC is the scoring path's pair form (gemm_f32.hip "f32 x3", the triple-plane linears of forward_f32): every f32 operand x is
// hi = bf16(x), lo = bf16(x - hi), and a product is hi hi + hi lo + lo hi on v_mfma_f32_16x16x32_bf16 into ONE f32 accumulator —
//   S  = K_hi Q_hi + K_hi Q_lo + K_lo Q_hi          Q split into registers when its rows are loaded; K, V split between the global load
//   O += V_hi P_hi + V_lo P_hi + V_hi P_lo          and the LDS write (the conversion rules out LDS-DMA); P = exp2(.) split in registers
// — 48 matrix instructions per wave and block against the bf16 kernel's 16.  P as plain bf16 would leave 2^-9 of error in O.
// Always the pair form: SCL_F32X3 (a switch of the GEMM entry points) does not reach this kernel.
//
// LDS: four images per block (K hi / lo as rows, V hi / lo transposed, 8 KiB each), double-buffered = 64 KiB per workgroup.
//
// THE STORES are those of the bf16 packed forward: no row at or beyond an utterance's end is loaded or stored, a query block that starts
// beyond Tb leaves before its first barrier, rows [Mv, Mq) of ctx are written as zeros by every launch, rows >= Mq are never touched.
#include "attn_stream_body.h"
#include "attn_wide.h"      // head dims 72..128: scl_attn_wide_fwd_f32 (attention_f32_wide.hip)

namespace {

typedef __attribute__((ext_vector_type(8))) float f32x8a;

// eight f32 (two 16-byte vectors) -> the hi and lo bf16 planes, 16 bytes each (f32_split8 of gemm_f32.hip)
__device__ __forceinline__ void split8(const float4& a, const float4& b, uint4& hi, uint4& lo) {
    const f32x8a x = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const bf16x8 h = __builtin_convertvector(x, bf16x8);
    const f32x8a back = __builtin_convertvector(h, f32x8a);
    const bf16x8 l = __builtin_convertvector(x - back, bf16x8);
    hi = __builtin_bit_cast(uint4, h);
    lo = __builtin_bit_cast(uint4, l);
}

// the lane's query row as the B operand of both k steps, hi and lo planes (columns 32 ks + 8 g + 0..7; zeros past Tb)
__device__ __forceinline__ void q_load_split(const float* __restrict__ base, int64_t pitch, int q, int Tb, int g, bf16x8 (&qh)[2], bf16x8 (&ql)[2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (q < Tb) {
            const float4* src = reinterpret_cast<const float4*>(base + (int64_t)q * pitch + 32 * ks + 8 * g);
            a = src[0]; b = src[1];
        }
        uint4 h, l;
        split8(a, b, h, l);
        qh[ks] = __builtin_bit_cast(bf16x8, h);
        ql[ks] = __builtin_bit_cast(bf16x8, l);
    }
}

// K / V block staging in f32: 64 keys x 8 chunks of 8 floats of K and of V = 2 + 2 chunks (4 + 4 vectors) per thread, zeros for keys
// past Tb (their scores are masked; a zero V row keeps 0 x garbage out of the P V product).  The thread / chunk map is kv_fetch's, so
// the split planes go through kv_store unchanged.
struct KVRegsF { float4 k[2][2], v[2][2]; };
__device__ __forceinline__ void kvf_fetch(KVRegsF& r, const float* __restrict__ base, int64_t pitch, int E, int key0, int Tb) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = threadIdx.x + 256 * it, key = key0 + (idx >> 3), c = idx & 7;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        r.k[it][0] = z; r.k[it][1] = z; r.v[it][0] = z; r.v[it][1] = z;
        if (key < Tb) {
            const float4* ks = reinterpret_cast<const float4*>(base + (int64_t)key * pitch + E + 8 * c);
            const float4* vs = reinterpret_cast<const float4*>(base + (int64_t)key * pitch + 2 * E + 8 * c);
            r.k[it][0] = ks[0]; r.k[it][1] = ks[1];
            r.v[it][0] = vs[0]; r.v[it][1] = vs[1];
        }
    }
}
// buf: [K hi rows | K lo rows | V hi tr | V lo tr], LKB * 128 bytes each
__device__ __forceinline__ void kvf_store(const KVRegsF& r, char* buf) {
    KVRegs hi, lo;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        split8(r.k[it][0], r.k[it][1], hi.k[it], lo.k[it]);
        split8(r.v[it][0], r.v[it][1], hi.v[it], lo.v[it]);
    }
    kv_store(hi, buf, nullptr, nullptr, buf + 2 * LKB * 128);
    kv_store(lo, buf + LKB * 128, nullptr, nullptr, buf + 3 * LKB * 128);
}

__global__ __launch_bounds__(256, 2) void attn_fwd_packed_f32_kernel(const float* __restrict__ qkv, float* __restrict__ ctx,
                                                                     const int* __restrict__ row0, int T, int H, int nqb, int B, int Mq,
                                                                     float scale) {
    __shared__ __attribute__((aligned(16))) char smem[2][4 * LKB * 128];      // [buffer][K hi rows, K lo rows, V hi tr, V lo tr]
    const int E = H * LD;
    const int64_t pitch = 3 * (int64_t)E;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const UttRows<Rows::Packed> utt(row0, b, T, Mq);
    const int Tb = utt.Tb;      // one value per workgroup: everything that depends on it is workgroup-uniform
    const float* base = qkv + utt.r0 * pitch + h * LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, g = lane >> 4;
    const int q = qblk * LQB + 16 * wave + lc;
    zero_tail_vectors(reinterpret_cast<uint4*>(ctx), row0, B, Mq, E / 4);
    if (qblk * LQB >= Tb) return;      // these rows are another utterance's (or nobody's): out before any barrier, no store (uniform)
    const int nkb = (Tb + LKB - 1) / LKB;
    bf16x8 qh[2], ql[2];
    q_load_split(base, pitch, q, Tb, g, qh, ql);
    KVRegsF r;
    kvf_fetch(r, base, pitch, E, 0, Tb);
    kvf_store(r, smem[0]);
    __syncthreads();
    const float sl2 = scale * LOG2E;
    float m = -INFINITY, l = 0.f;      // running max (raw score units) and this lane's share of the running sum
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
        const int p = kb & 1;
        if (kb + 1 < nkb) kvf_fetch(r, base, pitch, E, (kb + 1) * LKB, Tb);      // in flight under this block's products
        const char* Kh = smem[p];
        const char* Kl = Kh + LKB * 128;
        const char* Vh = Kh + 2 * LKB * 128;
        const char* Vl = Kh + 3 * LKB * 128;
        const int key0 = kb * LKB;
        f32x4 s[4];
        float mb = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {      // small terms first, then hi hi
                const bf16x8 kh = l_frag_rows(Kh, t, ks, lane);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_rows(Kl, t, ks, lane), qh[ks], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql[ks], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh[ks], s[t], 0, 0, 0);
            }
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
        f32x4 sl[4];      // p - bf16(p)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][rr], sl2, msl));
                ls += pv;
                s[t][rr] = pv;
                sl[t][rr] = pv - bf2f(f2bf(pv));
            }
        l = l * alpha + ls;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bf16x8 ph = l_pack8(s[2 * u], s[2 * u + 1]);
            const bf16x8 pl = l_pack8(sl[2 * u], sl[2 * u + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16x8 vh = l_frag_tr(Vh, 32 * u, 32 * u + 16, dt, lane);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(l_frag_tr(Vl, 32 * u, 32 * u + 16, dt, lane), ph, o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pl, o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, ph, o[dt], 0, 0, 0);
            }
        }
        if (kb + 1 < nkb) kvf_store(r, smem[p ^ 1]);      // its last readers finished before the previous barrier
        __syncthreads();
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    if (q < Tb) {      // nothing is stored at or beyond Tb
        float* dst = ctx + (utt.r0 + q) * E + h * LD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<float4*>(dst + 16 * dt) = make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    }
}

}  // namespace

extern "C" int scl_attn_fwd_packed_f32(const float* qkv, float* ctx, const int32_t* row0, int B, int T, int H, int D, int Mq, float scale,
                                       void* stream) {
    SCL_REQUIRE(qkv && ctx && row0 && B > 0 && H > 0 && T >= 1, "attn_fwd_packed_f32: bad args");
    SCL_REQUIRE(D == LD || scl_attn_wide_takes(D), "attn_fwd_packed_f32: " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);
    SCL_REQUIRE(Mq >= B && Mq % 64 == 0 && (int64_t)Mq <= ((int64_t)B * T + 63) / 64 * 64,
                "attn_fwd_packed_f32: need B <= Mq <= roundup(B * T, 64), a multiple of 64 (got Mq=%d)", Mq);
    SCL_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)ctx & 15) == 0, "attn_fwd_packed_f32: qkv and ctx must be 16-byte aligned");
    const int nqb = (T + LQB - 1) / LQB;
    SCL_REQUIRE((int64_t)B * H * nqb < 0x7FFFFFFF, "attn_fwd_packed_f32: grid too large");
    if (D != LD) return scl_attn_wide_fwd_f32(qkv, ctx, row0, B, T, H, D, Mq, scale, stream);
    hipLaunchKernelGGL(attn_fwd_packed_f32_kernel, dim3((unsigned)(B * H * nqb)), dim3(256), 0, (hipStream_t)stream, qkv, ctx, (const int*)row0,
                       T, H, nqb, B, Mq, scale);
    return scl_check_launch("scl_attn_fwd_packed_f32");
}
