// attn_tiles.h — LDS tile images, MFMA operand fragments and the K / V block staging shared by the streaming attention kernels
// (attn_stream_body.h: the forward / backward bodies behind the fixed-length kernels of attention_long.hip, the padded layout of
// attention_varlen.hip and the packed one of attention_packed.hip; attention_f32.hip: the fp32 packed forward).
// Everything is internal to the including file (anonymous namespace, force-inlined).
#pragma once
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((address_space(3))) s16x4 lds_s16x4_l;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4l;

// LDS images of a [rows][64] bf16 tile, 128-byte rows (the same two images as attention.hip's fused kernels):
// row image for ds_read_b128 row reads, 16-byte slot ^= (row >> 1) & 7; tr image for ds_read_b64_tr_b16, 32-byte chunk ^= (row >> 1) & 3
__device__ __forceinline__ int lk_off(int row, int c) { return row * 128 + ((c ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int lt_off(int row, int d) { return row * 128 + ((((d >> 4) ^ ((row >> 1) & 3))) << 5) + ((d & 15) << 1); }

// operand fragment of 16 rows (rowblk) x 32 columns (k step ks): lane holds row 16 rowblk + (lane & 15), columns 32 ks + 8 (lane >> 4) + 0..7
__device__ __forceinline__ bf16x8 l_frag_rows(const char* tile, int rowblk, int ks, int lane) {
    const int row = rowblk * 16 + (lane & 15);
    return *reinterpret_cast<const bf16x8*>(tile + lk_off(row, 4 * ks + (lane >> 4)));
}
// transposed operand [i = d (16, block dt)][k = 8 rows]: rows rowa + 4g + 0..3 and rowb + 4g + 0..3 — the k order of a packed pair of
// accumulator tiles (rows 4g + r of tile a, then of tile b).  Every lane of the wave must execute it (cross-lane gather).
__device__ __forceinline__ bf16x8 l_frag_tr(const char* tile, int rowa, int rowb, int dt, int lane) {
    const int i = lane & 15, g = lane >> 4;
    const int ra = rowa + 4 * g + (i >> 2), rb = rowb + 4 * g + (i >> 2);
    const int col = 16 * dt + 4 * (i & 3);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_l*)(tile + lt_off(ra, col)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_l*)(tile + lt_off(rb, col)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ bf16x8 l_pack8(const f32x4& a, const f32x4& b) {
    u32x4l pk;
    pk[0] = pack_bf2(a[0], a[1]); pk[1] = pack_bf2(a[2], a[3]); pk[2] = pack_bf2(b[0], b[1]); pk[3] = pack_bf2(b[2], b[3]);
    return __builtin_bit_cast(bf16x8, pk);
}
// 16 rows of a [T][64] bf16 matrix (row pitch `pitch`) as an MFMA operand straight from global memory: the lane passes its own row q
// (first row + (lane & 15)) and receives columns 32 ks + 8 (lane >> 4) + 0..7 (zeros past T)
__device__ __forceinline__ void l_load_rows(const bf16_t* __restrict__ base, int64_t pitch, int q, int T, int g, bf16x8 (&f)[2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        uint4 u = make_uint4(0, 0, 0, 0);
        if (q < T) u = *reinterpret_cast<const uint4*>(base + (int64_t)q * pitch + 32 * ks + 8 * g);
        f[ks] = __builtin_bit_cast(bf16x8, u);
    }
}

// K / V block staging for the forward and dQ kernels: 64 keys x 8 16-byte chunks of K and of V = 2 + 2 vectors per thread (256 threads),
// zeros for keys past T (their scores are masked; a zero V row keeps 0 x garbage out of the P V product)
struct KVRegs { uint4 k[2], v[2]; };
__device__ __forceinline__ void kv_fetch(KVRegs& r, const bf16_t* __restrict__ base, int64_t pitch, int E, int key0, int T) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = threadIdx.x + 256 * it, key = key0 + (idx >> 3), c = idx & 7;
        r.k[it] = make_uint4(0, 0, 0, 0); r.v[it] = make_uint4(0, 0, 0, 0);
        if (key < T) {
            r.k[it] = *reinterpret_cast<const uint4*>(base + (int64_t)key * pitch + E + 8 * c);
            r.v[it] = *reinterpret_cast<const uint4*>(base + (int64_t)key * pitch + 2 * E + 8 * c);
        }
    }
}
// Kr: K row image, Kt: K tr image (nullptr = not wanted), Vr: V row image (nullptr = not wanted), Vt: V tr image (nullptr = not wanted)
__device__ __forceinline__ void kv_store(const KVRegs& r, char* Kr, char* Kt, char* Vr, char* Vt) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = threadIdx.x + 256 * it, key = idx >> 3, c = idx & 7;
        *reinterpret_cast<uint4*>(Kr + lk_off(key, c)) = r.k[it];
        if (Kt) *reinterpret_cast<uint4*>(Kt + lt_off(key, 8 * c)) = r.k[it];
        if (Vr) *reinterpret_cast<uint4*>(Vr + lk_off(key, c)) = r.v[it];
        if (Vt) *reinterpret_cast<uint4*>(Vt + lt_off(key, 8 * c)) = r.v[it];
    }
}

// Query tile staging for the dK / dV kernels, 32 rows per step: Q rows, Q tr, dO rows, dO tr images (4 KiB each), then lse (x log2 e) and delta of the 32 rows.
constexpr int QT_BYTES = 4 * 4096 + 2 * 32 * 4;

struct QRegs { uint4 q, o; float ls, dl; };
// thread i: query row i >> 3 of the tile, 16-byte chunk i & 7 (256 threads = 32 rows x 8 chunks); rows past T: zeros, lse = +huge (P = 0)
__device__ __forceinline__ void qt_fetch(QRegs& r, const bf16_t* __restrict__ base, int64_t pitch, const bf16_t* __restrict__ dob, int E,
                                         const float* __restrict__ lse_bh, const float* __restrict__ del_bh, int q0, int T) {
    const int row = threadIdx.x >> 3, c = threadIdx.x & 7, q = q0 + row;
    r.q = make_uint4(0, 0, 0, 0); r.o = make_uint4(0, 0, 0, 0); r.ls = 1e30f; r.dl = 0.f;
    if (q < T) {
        r.q = *reinterpret_cast<const uint4*>(base + (int64_t)q * pitch + 8 * c);
        r.o = *reinterpret_cast<const uint4*>(dob + (int64_t)q * E + 8 * c);
        if (c == 0) { r.ls = lse_bh[q] * LOG2E; r.dl = del_bh[q]; }
    }
}
__device__ __forceinline__ void qt_store(const QRegs& r, char* tile) {
    const int row = threadIdx.x >> 3, c = threadIdx.x & 7;
    *reinterpret_cast<uint4*>(tile + lk_off(row, c)) = r.q;
    *reinterpret_cast<uint4*>(tile + 4096 + lt_off(row, 8 * c)) = r.q;
    *reinterpret_cast<uint4*>(tile + 8192 + lk_off(row, c)) = r.o;
    *reinterpret_cast<uint4*>(tile + 12288 + lt_off(row, 8 * c)) = r.o;
    if (c == 0) {
        float* ld = reinterpret_cast<float*>(tile + 16384);
        ld[row] = r.ls; ld[32 + row] = r.dl;
    }
}

}  // namespace
