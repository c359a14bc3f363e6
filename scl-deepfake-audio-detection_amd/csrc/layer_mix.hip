// layer_mix.hip — the learned soft-max-weighted sum over all hidden states of the encoder (YAML `ssl_layer_mix`):
//   mix = sum_l s_l h_l,  s = softmax(a),  a: f32 [nstates] logits (nstates = layers + 1 <= SCL_LAYER_MIX_MAX_STATES),
//   h_0 .. h_{L-1} the f32 residual stream entering layer l (h_0: the positional-conv residual), h_L the final LayerNorm's output.
// Four HBM-bound kernels over flat [n = rows * E] arrays (n % 8 == 0: 16-byte accesses throughout):
//   fwd     bf16 mix from a table of the nstates f32 buffers, f32 accumulation in index order (training, bf16 scoring)
//   acc_f32 acc (+)= s_l h, the fp32 scoring path's one-layer-at-a-time form
//   bwd_w   the nstates dot products <g, h_l> (fp64 partial per block, summed in block order by a one-block finish that applies the
//           soft-max Jacobian and overwrites d(a)), and s_L g for the final LayerNorm's backward, in the same pass
//   inject  dx += s_l g on the f32 residual gradient, bf16 companion rewritten with the mask scl_layernorm_bwd gave it
// Every kernel recomputes the soft-max of the <= 64 logits itself (mix_weights: one code path, so all four agree to the bit); no
// atomics, no host synchronisation, every summation order fixed by (n, nstates) alone.
#include "common.h"

namespace {

constexpr int MAXS = SCL_LAYER_MIX_MAX_STATES;

struct MixTable { const float* h[MAXS]; };

// s_d[0 .. S) = softmax(logits) in fp64 and s_w = its rounding to f32 (so a weight is off by half an ulp, and every product s_l x by one
// rounding more), in LDS, by the first S threads of the block; max and sum run serially in index order.  64 exponentials per block: free
// beside the block's memory traffic.  Ends with a barrier.
__device__ __forceinline__ void mix_weights(const float* __restrict__ logits, int S, double* s_d, float* s_w) {
    const int t = threadIdx.x;
    if (t < S) s_d[t] = (double)logits[t];
    __syncthreads();
    double e = 0.0;
    if (t < S) {
        double mx = s_d[0];
        for (int l = 1; l < S; ++l) mx = fmax(mx, s_d[l]);
        e = exp(s_d[t] - mx);
    }
    __syncthreads();
    if (t < S) s_d[t] = e;
    __syncthreads();
    double sum = 0.0;
    if (t < S)
        for (int l = 0; l < S; ++l) sum += s_d[l];
    __syncthreads();
    if (t < S) {
        s_d[t] = e / sum;
        s_w[t] = (float)s_d[t];
    }
    __syncthreads();
}

__device__ __forceinline__ void ld8(const float* __restrict__ p, int64_t i, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p + i);
    const float4 b = *reinterpret_cast<const float4*>(p + i + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void ld8_bf(const bf16_t* __restrict__ p, int64_t i, float* v) {
    const uint4 u = *reinterpret_cast<const uint4*>(p + i);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = __uint_as_float(w[k] << 16); v[2 * k + 1] = __uint_as_float(w[k] & 0xFFFF0000u); }
}
template <bool F32>
__device__ __forceinline__ void ld8_any(const void* __restrict__ p, int64_t i, float* v) {
    if (F32) ld8(static_cast<const float*>(p), i, v);
    else ld8_bf(static_cast<const bf16_t*>(p), i, v);
}
__device__ __forceinline__ void st8(float* __restrict__ p, int64_t i, const float* v) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void st8_bf(bf16_t* __restrict__ p, int64_t i, const float* v) {
    uint4 u;
    u.x = pack_bf2(v[0], v[1]); u.y = pack_bf2(v[2], v[3]); u.z = pack_bf2(v[4], v[5]); u.w = pack_bf2(v[6], v[7]);
    *reinterpret_cast<uint4*>(p + i) = u;
}

// ---- forward: one pass over the table ------------------------------------------------------------------------------------------------
// A thread owns 8 consecutive elements; the states are walked four at a time so that eight 16-byte loads are in flight per thread.
__global__ __launch_bounds__(256) void layer_mix_fwd_kernel(MixTable tab, int S, const float* __restrict__ logits, bf16_t* __restrict__ mix,
                                                            int64_t n) {
    __shared__ double s_d[MAXS];
    __shared__ float s_w[MAXS];
    mix_weights(logits, S, s_d, s_w);
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= n) return;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    int l = 0;
    for (; l + 4 <= S; l += 4) {
        float v[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j) ld8(tab.h[l + j], i, v[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = s_w[l + j];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = __builtin_fmaf(s, v[j][k], acc[k]);
        }
    }
    for (; l < S; ++l) {
        float v[8];
        ld8(tab.h[l], i, v);
        const float s = s_w[l];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = __builtin_fmaf(s, v[k], acc[k]);
    }
    st8_bf(mix, i, acc);
}

// ---- fp32 scoring: acc (+)= s_index h ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layer_mix_acc_kernel(const float* __restrict__ h, const float* __restrict__ logits, int S, int index,
                                                            float* __restrict__ acc, int accumulate, int64_t n) {
    __shared__ double s_d[MAXS];
    __shared__ float s_w[MAXS];
    mix_weights(logits, S, s_d, s_w);
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= n) return;
    const float s = s_w[index];
    float v[8], a[8];
    ld8(h, i, v);
    if (accumulate) ld8(acc, i, a);
    else {
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = __builtin_fmaf(s, v[k], a[k]);
    st8(acc, i, a);
}

// ---- backward, the logits --------------------------------------------------------------------------------------------------------------------
// A block owns BWD_TILE consecutive elements: a thread keeps its 8 * BWD_IT values of g in registers, walks the states, and sums its
// products in fp64; lanes, then waves, then (finish kernel) blocks are combined in fixed order.  part: f64 [nblocks][S].
constexpr int BWD_IT = 4;
constexpr int BWD_TILE = 256 * 8 * BWD_IT;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <bool GF32>
__global__ __launch_bounds__(256) void layer_mix_bwd_w_kernel(const void* __restrict__ g, MixTable tab, int S, const float* __restrict__ logits,
                                                              float* __restrict__ g_last, double* __restrict__ part, int64_t n) {
    __shared__ double s_d[MAXS];
    __shared__ float s_w[MAXS];
    __shared__ double red[MAXS][4];
    mix_weights(logits, S, s_d, s_w);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * BWD_TILE + (int64_t)threadIdx.x * 8;
    float gv[BWD_IT][8];
    const float sl = s_w[S - 1];
#pragma unroll
    for (int it = 0; it < BWD_IT; ++it) {
        const int64_t i = base + (int64_t)it * 2048;
        if (i < n) {
            ld8_any<GF32>(g, i, gv[it]);
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = sl * gv[it][k];
            st8(g_last, i, o);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) gv[it][k] = 0.f;
        }
    }
    for (int l = 0; l < S; ++l) {
        const float* __restrict__ h = tab.h[l];
        float hv[BWD_IT][8];
#pragma unroll
        for (int it = 0; it < BWD_IT; ++it) {
            const int64_t i = base + (int64_t)it * 2048;
            if (i < n) ld8(h, i, hv[it]);
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) hv[it][k] = 0.f;
            }
        }
        double acc = 0.0;
#pragma unroll
        for (int it = 0; it < BWD_IT; ++it)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fma((double)gv[it][k], (double)hv[it][k], acc);
        acc = wave_sum_f64(acc);
        if (lane == 0) red[l][w] = acc;
    }
    __syncthreads();
    if (threadIdx.x < S) {
        const int l = threadIdx.x;
        part[(int64_t)blockIdx.x * S + l] = ((red[l][0] + red[l][1]) + red[l][2]) + red[l][3];
    }
}

// One block of 16 * MAXS threads: 16 lanes per state sum the block partials b = sub, sub + 16, ... in order, the 16 sums are combined in
// lane order; then da = s o (dS - sum_l s_l dS_l) in fp64, stored as f32.
__global__ __launch_bounds__(16 * MAXS) void layer_mix_bwd_w_finish_kernel(const double* __restrict__ part, int nblocks, int S,
                                                                           const float* __restrict__ logits, float* __restrict__ da) {
    __shared__ double s_d[MAXS];
    __shared__ float s_w[MAXS];
    __shared__ double sub_sum[MAXS][16];
    __shared__ double dS[MAXS];
    mix_weights(logits, S, s_d, s_w);
    const int l = threadIdx.x >> 4, sub = threadIdx.x & 15;
    double acc = 0.0;
    if (l < S)
        for (int b = sub; b < nblocks; b += 16) acc += part[(int64_t)b * S + l];
    sub_sum[l][sub] = acc;
    __syncthreads();
    if (sub == 0 && l < S) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += sub_sum[l][k];
        dS[l] = t;
    }
    __syncthreads();
    if (threadIdx.x < S) {
        double dot = 0.0;
        for (int k = 0; k < S; ++k) dot += s_d[k] * dS[k];
        da[threadIdx.x] = (float)(s_d[threadIdx.x] * (dS[threadIdx.x] - dot));
    }
}

// ---- backward, the residual stream ------------------------------------------------------------------------------------------------------
template <bool GF32>
__global__ __launch_bounds__(256) void layer_mix_inject_kernel(const void* __restrict__ g, const float* __restrict__ logits, int S, int index,
                                                               float* __restrict__ dx, bf16_t* __restrict__ dx_bf, int64_t n, uint32_t seed,
                                                               float p) {
    __shared__ double s_d[MAXS];
    __shared__ float s_w[MAXS];
    mix_weights(logits, S, s_d, s_w);
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= n) return;
    const float s = s_w[index];
    float gv[8], o[8];
    ld8_any<GF32>(g, i, gv);
    ld8(dx, i, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = __builtin_fmaf(s, gv[k], o[k]);
    st8(dx, i, o);
    if (dx_bf) {
        if (p > 0.f) {      // the `dout` mask of scl_layernorm_bwd: element index = row * E + column = the flat index
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] *= dropout_scale(seed, (uint64_t)(i + k), p);
        }
        st8_bf(dx_bf, i, o);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int fill_table(MixTable& tab, const float* const* states, int S) {
    for (int l = 0; l < MAXS; ++l) tab.h[l] = nullptr;
    for (int l = 0; l < S; ++l) {
        if (!states[l] || !aligned16(states[l])) return -1;
        tab.h[l] = states[l];
    }
    return 0;
}

inline int64_t bwd_blocks(int64_t n) { return (n + BWD_TILE - 1) / BWD_TILE; }

}  // namespace

#define MIX_COMMON(what)                                                                                                          \
    SCL_REQUIRE(nstates >= 1 && nstates <= MAXS, what ": 1 .. %d hidden states, got %d", MAXS, nstates);                           \
    SCL_REQUIRE(logits && n > 0 && n % 8 == 0 && (n + 2047) / 2048 < (int64_t)0x7FFFFFFF, what ": n must be a positive multiple of 8")

extern "C" int scl_layer_mix_fwd(const float* const* states, int nstates, const float* logits, void* mix_bf16, int64_t n, void* stream) {
    MIX_COMMON("layer_mix_fwd");
    MixTable tab;
    SCL_REQUIRE(states && mix_bf16 && aligned16(mix_bf16) && fill_table(tab, states, nstates) == 0,
                "layer_mix_fwd: null or unaligned pointer (16 bytes)");
    hipLaunchKernelGGL(layer_mix_fwd_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tab, nstates, logits,
                       (bf16_t*)mix_bf16, n);
    return scl_check_launch("scl_layer_mix_fwd");
}

extern "C" int scl_layer_mix_acc_f32(const float* h, const float* logits, int nstates, int index, float* acc, int accumulate, int64_t n,
                                     void* stream) {
    MIX_COMMON("layer_mix_acc_f32");
    SCL_REQUIRE(index >= 0 && index < nstates, "layer_mix_acc_f32: state index %d outside 0 .. %d", index, nstates - 1);
    SCL_REQUIRE(h && acc && aligned16(h) && aligned16(acc), "layer_mix_acc_f32: null or unaligned pointer (16 bytes)");
    hipLaunchKernelGGL(layer_mix_acc_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h, logits, nstates, index,
                       acc, accumulate, n);
    return scl_check_launch("scl_layer_mix_acc_f32");
}

extern "C" long long scl_layer_mix_bwd_w_ws_bytes(int64_t n, int nstates) {
    if (n <= 0 || nstates < 1 || nstates > MAXS) return 0;
    return (long long)(bwd_blocks(n) * nstates * (int64_t)sizeof(double));
}

extern "C" int scl_layer_mix_bwd_w(const void* g, int g_f32, const float* const* states, int nstates, const float* logits, float* g_last,
                                   void* ws, float* d_logits, int64_t n, void* stream) {
    MIX_COMMON("layer_mix_bwd_w");
    MixTable tab;
    SCL_REQUIRE(g && states && g_last && ws && d_logits && aligned16(g) && aligned16(g_last) && aligned16(ws) &&
                fill_table(tab, states, nstates) == 0, "layer_mix_bwd_w: null or unaligned pointer (16 bytes)");
    const int64_t nb = bwd_blocks(n);
    if (g_f32) hipLaunchKernelGGL(layer_mix_bwd_w_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, g, tab, nstates, logits,
                                  g_last, (double*)ws, n);
    else hipLaunchKernelGGL(layer_mix_bwd_w_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, g, tab, nstates, logits,
                            g_last, (double*)ws, n);
    hipLaunchKernelGGL(layer_mix_bwd_w_finish_kernel, dim3(1), dim3(16 * MAXS), 0, (hipStream_t)stream, (const double*)ws, (int)nb, nstates,
                       logits, d_logits);
    return scl_check_launch("scl_layer_mix_bwd_w");
}

extern "C" int scl_layer_mix_bwd_inject(const void* g, int g_f32, const float* logits, int nstates, int index, float* dx, void* dx_bf16,
                                        int64_t n, uint32_t seed, float p, void* stream) {
    MIX_COMMON("layer_mix_bwd_inject");
    SCL_REQUIRE(index >= 0 && index < nstates, "layer_mix_bwd_inject: state index %d outside 0 .. %d", index, nstates - 1);
    SCL_REQUIRE(p >= 0.f && p < 1.f, "layer_mix_bwd_inject: dropout probability in [0, 1)");
    SCL_REQUIRE(g && dx && aligned16(g) && aligned16(dx) && aligned16(dx_bf16), "layer_mix_bwd_inject: null or unaligned pointer (16 bytes)");
    const dim3 grid((unsigned)((n / 8 + 255) / 256));
    if (g_f32) hipLaunchKernelGGL(layer_mix_inject_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g, logits, nstates, index, dx,
                                  (bf16_t*)dx_bf16, n, seed, p);
    else hipLaunchKernelGGL(layer_mix_inject_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g, logits, nstates, index, dx,
                            (bf16_t*)dx_bf16, n, seed, p);
    return scl_check_launch("scl_layer_mix_bwd_inject");
}
