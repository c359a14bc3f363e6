// gat.hip — the pairwise attention score of the AASIST graph-attention layers, forward and backward, fused.
//
//   s[b][i][j] = sum_o tanh( sum_d W[o][d] * x[b][i][d] * x[b][j][d] + bias[o] ) * a_t(i,j)[o]
//
// is what GraphAttentionLayer._derive_att_map / HtrgGraphAttentionLayer._derive_att_map compute before the temperature and
// the softmax (model/wav2vec2_aasist.py:107-135, 259-291): `att_proj` applied to the element-wise product of every node
// pair, tanh, and a dot with `att_weight` — for the heterogeneous layer one of three vectors chosen by the types of the
// two nodes (a11 both < n1, a22 both >= n1, a12 mixed).  The reference materialises [B, N, N, D] and [B, N, N, D'] tensors
// and runs fp32 library GEMMs with M = B*N*N rows on them (15 TFLOP/s, ~6 ms of the 16 ms the torch-composed back-end
// costs per step); here a thread owns one node pair, W / x live in LDS, and nothing of size N*N*D ever reaches HBM in the
// forward.  All arithmetic is fp32 (the back-end's parity bar is the fp32 one).
//
// Backward (given ds): recompute h per pair, then
//   d a_t[o]  = sum_{pairs of type t} ds * h_o                       (wave reductions -> per-block partials)
//   d pre_o   = ds * a_t[o] * (1 - h_o^2);  d bias[o] = sum d pre_o
//   d W[o][d] = sum_pairs d pre_o * x_i[d] x_j[d]                    (d pre tile in LDS, 16 outputs per thread)
//   d p[d]    = sum_o d pre_o W[o][d]  -> dP[b][i][j][d] in HBM (the only N*N*D tensor), gathered by a second kernel into
//   d x_i[d]  = sum_j (dP[i][j][d] + dP[j][i][d]) * x_j[d]           (deterministic: no atomics anywhere)
//
// Graph sizes: up to GAT_MAXN = 128 nodes the kernels keep a whole graph's x in LDS; 129 .. GAT_CAP = 1024 nodes (clips beyond 387 frames:
// nT = T / 3 temporal nodes) run the tiled matrix-core forms further down, whose LDS does not grow with N.
#include "common.h"

namespace {

constexpr int GAT_MAXN = 128;     // nodes per graph of the whole-graph-in-LDS kernels (and of the scalar forms' byte-wide pair indices)
constexpr int GAT_CAP = 1024;     // nodes per graph of the tiled matrix-core forms (999 temporal nodes: a 960,000-sample clip)
constexpr int GAT_JT = 128;       // tiled forms: nodes j staged per tile
constexpr int GAT_IPB = 8;        // tiled forms: nodes i a block owns (at most)
constexpr int GAT_PAIRS = 256;    // pairs (= threads) per block
constexpr int GAT_DPS = 68;       // row stride (floats) of the backward's d-pre tile [pair][o]: 16-byte aligned, 4-way banked

template <int D>
struct GatSmem {
    // W [Do][D] | bias [Do] | a [3][Do] | x [N][D+1]
    __device__ static float* w(float* s) { return s; }
    __device__ static float* bias(float* s, int Do) { return s + Do * D; }
    __device__ static float* a(float* s, int Do) { return s + Do * D + Do; }
    __device__ static float* x(float* s, int Do) { return s + Do * D + 4 * Do; }
    __host__ __device__ static size_t floats(int Do, int N) { return (size_t)Do * D + 4 * Do + (size_t)N * (D + 1); }
};

template <int D>
__device__ __forceinline__ void gat_stage(float* sm, const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                          const float* __restrict__ a, int b, int N, int Do) {
    float* w = GatSmem<D>::w(sm);
    for (int i = threadIdx.x; i < Do * D; i += blockDim.x) w[i] = W[i];
    float* bs = GatSmem<D>::bias(sm, Do);
    float* as = GatSmem<D>::a(sm, Do);
    for (int i = threadIdx.x; i < Do; i += blockDim.x) bs[i] = bias[i];
    for (int i = threadIdx.x; i < 3 * Do; i += blockDim.x) as[i] = a[i];
    float* xs = GatSmem<D>::x(sm, Do);
    const float* xb = x + (int64_t)b * N * D;
    for (int i = threadIdx.x; i < N * D; i += blockDim.x) xs[(i / D) * (D + 1) + (i % D)] = xb[i];
}

__device__ __forceinline__ int gat_type(int i, int j, int n1) { return (i < n1) == (j < n1) ? (i < n1 ? 0 : 1) : 2; }

__device__ __forceinline__ float gat_tanh(float v) {
    // tanh(v) = 1 - 2 / (exp(2v) + 1): |err| < 2 ulp of fp32 over the whole range, saturates cleanly
    const float e = __expf(2.0f * v);
    return 1.0f - 2.0f / (e + 1.0f);
}

template <int D>
__global__ __launch_bounds__(GAT_PAIRS) void gat_score_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                  const float* __restrict__ bias, const float* __restrict__ a,
                                                                  float* __restrict__ s, int N, int Do, int n1) {
    extern __shared__ float sm[];
    const int b = blockIdx.y;
    gat_stage<D>(sm, x, W, bias, a, b, N, Do);
    __syncthreads();
    const int q = blockIdx.x * GAT_PAIRS + threadIdx.x;
    if (q >= N * N) return;
    const int i = q / N, j = q - i * N;
    const float* w = GatSmem<D>::w(sm);
    const float* bs = GatSmem<D>::bias(sm, Do);
    const float* at = GatSmem<D>::a(sm, Do) + gat_type(i, j, n1) * Do;
    const float* xi = GatSmem<D>::x(sm, Do) + i * (D + 1);
    const float* xj = GatSmem<D>::x(sm, Do) + j * (D + 1);
    float p[D];
#pragma unroll
    for (int d = 0; d < D; ++d) p[d] = xi[d] * xj[d];
    float acc = 0.f;
    for (int o = 0; o < Do; ++o) {
        float pre = bs[o];
        const float4* wr = reinterpret_cast<const float4*>(w + o * D);
#pragma unroll
        for (int d4 = 0; d4 < D / 4; ++d4) {
            const float4 ww = wr[d4];
            pre += ww.x * p[4 * d4] + ww.y * p[4 * d4 + 1] + ww.z * p[4 * d4 + 2] + ww.w * p[4 * d4 + 3];
        }
        acc += gat_tanh(pre) * at[o];
    }
    s[(int64_t)b * N * N + q] = acc;
}

// part[blk] = [ dW (Do*D) | dbias (Do) | da (3*Do) ] ; dP[b][q][d]
template <int D>
__global__ __launch_bounds__(GAT_PAIRS) void gat_score_bwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                  const float* __restrict__ bias, const float* __restrict__ a,
                                                                  const float* __restrict__ ds, float* __restrict__ dP,
                                                                  float* __restrict__ part, int N, int Do, int n1) {
    extern __shared__ float sm[];
    const int b = blockIdx.y;
    gat_stage<D>(sm, x, W, bias, a, b, N, Do);
    float* dpre_l = sm + ((GatSmem<D>::floats(Do, N) + 3) & ~(size_t)3);   // [GAT_PAIRS][GAT_DPS]
    float* red = dpre_l + (size_t)GAT_PAIRS * GAT_DPS;          // [4 waves][Do][4]  (-, da0, da1, da2)
    unsigned char* pi = reinterpret_cast<unsigned char*>(red + 4 * Do * 4);   // [GAT_PAIRS] i, then [GAT_PAIRS] j
    unsigned char* pj = pi + GAT_PAIRS;
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x * GAT_PAIRS + tid;
    const bool valid = q < N * N;
    const int i = valid ? q / N : 0, j = valid ? q - i * N : 0;
    pi[tid] = (unsigned char)i; pj[tid] = (unsigned char)j;
    const int ty = gat_type(i, j, n1);
    const float* w = GatSmem<D>::w(sm);
    const float* bs = GatSmem<D>::bias(sm, Do);
    const float* at = GatSmem<D>::a(sm, Do) + ty * Do;
    const float* xs = GatSmem<D>::x(sm, Do);
    const float* xi = xs + i * (D + 1);
    const float* xj = xs + j * (D + 1);
    const float g = valid ? ds[(int64_t)b * N * N + q] : 0.f;
    float p[D], dp[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { p[d] = xi[d] * xj[d]; dp[d] = 0.f; }
    for (int o = 0; o < Do; ++o) {
        float pre = bs[o];
        const float4* wr = reinterpret_cast<const float4*>(w + o * D);
#pragma unroll
        for (int d4 = 0; d4 < D / 4; ++d4) {
            const float4 ww = wr[d4];
            pre += ww.x * p[4 * d4] + ww.y * p[4 * d4 + 1] + ww.z * p[4 * d4 + 2] + ww.w * p[4 * d4 + 3];
        }
        const float h = gat_tanh(pre);
        const float dpre = g * at[o] * (1.0f - h * h);
        dpre_l[tid * GAT_DPS + o] = dpre;
#pragma unroll
        for (int d4 = 0; d4 < D / 4; ++d4) {
            const float4 ww = wr[d4];
            dp[4 * d4] += dpre * ww.x; dp[4 * d4 + 1] += dpre * ww.y; dp[4 * d4 + 2] += dpre * ww.z; dp[4 * d4 + 3] += dpre * ww.w;
        }
        // per-wave sums of ds*h by pair type (fixed order: deterministic); the homogeneous layer has one type
        const float gh = g * h;
        const float r1 = wave_sum(ty == 0 ? gh : 0.f);
        float r2 = 0.f, r3 = 0.f;
        if (n1 < N) { r2 = wave_sum(ty == 1 ? gh : 0.f); r3 = wave_sum(ty == 2 ? gh : 0.f); }
        if (lane == 0) {
            float* r = red + (wave * Do + o) * 4;
            r[1] = r1; r[2] = r2; r[3] = r3;
        }
    }
    if (valid) {
        float* out = dP + ((int64_t)b * N * N + q) * D;
#pragma unroll
        for (int d4 = 0; d4 < D / 4; ++d4)
            *reinterpret_cast<float4*>(out + 4 * d4) = make_float4(dp[4 * d4], dp[4 * d4 + 1], dp[4 * d4 + 2], dp[4 * d4 + 3]);
    }
    __syncthreads();
    float* pb = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ((size_t)Do * D + 4 * Do);
    // ---- dW[o][d] = sum_pairs dpre[pair][o] * x_i[d] x_j[d]: thread -> (d = tid % D, 16 consecutive o); the whole wave shares the
    //      d-pre addresses (LDS broadcast), x reads are conflict-free across d; dbias[o] = sum_pairs dpre[pair][o] from the same pass
    {
        const int d = tid % D, og = tid / D;
        for (int o0 = og * 16; o0 < Do; o0 += (GAT_PAIRS / D) * 16) {
            float accw[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) accw[t] = 0.f;
            for (int pr = 0; pr < GAT_PAIRS; ++pr) {
                const float pv = xs[pi[pr] * (D + 1) + d] * xs[pj[pr] * (D + 1) + d];
                const float4* dr = reinterpret_cast<const float4*>(dpre_l + pr * GAT_DPS + o0);
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const float4 dv = dr[t4];
                    accw[4 * t4] += dv.x * pv; accw[4 * t4 + 1] += dv.y * pv; accw[4 * t4 + 2] += dv.z * pv; accw[4 * t4 + 3] += dv.w * pv;
                }
            }
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (o0 + t < Do) pb[(o0 + t) * D + d] = accw[t];
        }
    }
    // ---- dbias[o] (row sums of the d-pre tile) and da: combine the 4 waves
    for (int o = tid; o < Do; o += GAT_PAIRS) {
        float sb = 0.f;
        for (int pr = 0; pr < GAT_PAIRS; ++pr) sb += dpre_l[pr * GAT_DPS + o];
        pb[(size_t)Do * D + o] = sb;
    }
    for (int t = tid; t < Do * 3; t += GAT_PAIRS) {
        const int o = t / 3, c = 1 + t % 3;
        const float v = red[(0 * Do + o) * 4 + c] + red[(1 * Do + o) * 4 + c] + red[(2 * Do + o) * 4 + c] + red[(3 * Do + o) * 4 + c];
        pb[(size_t)Do * D + Do + (c - 1) * Do + o] = v;
    }
}

// dx[b][i][d] = sum_j (dP[b][i][j][d] + dP[b][j][i][d]) * x[b][j][d];  one block per (b, i), threads = 4 j-lanes x D
// VAR: N is the batch's Nmax (the strides of x, dx and of the utterance's dP block), the sums run over the utterance's own nodes[b] nodes of
// its own [N_b][N_b][D] matrix at the start of the block, and a row i >= N_b is written as zeros (the whole block: before the barrier).
template <int D, bool VAR = false>
__global__ void gat_dx_kernel(const float* __restrict__ dP, const float* __restrict__ x, float* __restrict__ dx, int N, const int* __restrict__ nodes = nullptr) {
    __shared__ float red[4][D];
    const int b = blockIdx.y, i = blockIdx.x;
    const int d = threadIdx.x % D, jl = threadIdx.x / D;
    const float* xb = x + (int64_t)b * N * D;
    const float* pb = dP + (int64_t)b * N * N * D;
    float* dxr = dx + ((int64_t)b * N + i) * D;
    if (VAR) {
        const int Nmax = N;
        N = nodes[b]; N = N < 1 ? 1 : (N > Nmax ? Nmax : N);
        if (i >= N) { if (jl == 0) dxr[d] = 0.f; return; }
    }
    float s = 0.f;
    for (int j = jl; j < N; j += 4)
        s += (pb[((int64_t)i * N + j) * D + d] + pb[((int64_t)j * N + i) * D + d]) * xb[(int64_t)j * D + d];
    red[jl][d] = s;
    __syncthreads();
    if (jl == 0) dxr[d] = red[0][d] + red[1][d] + red[2][d] + red[3][d];
}

// ---- matrix-core forms (D in {32, 64}, Do in {32, 64}) ----------------------------------------------------------------------------------
// The pre-activation of a pair is a [pairs x D] x [D x Do] product whose left operand is formed on the fly (x_i * x_j): on
// v_mfma_f32_16x16x4_f32 (exact fp32) a wave takes one node i and 16 nodes j at a time — rows = the 16 pairs, k = the feature index,
// columns = 16 outputs — with the whole of W in registers (Do * D / 64 per lane, loaded once per block), so the N * N * D * Do
// multiply-adds leave the vector ALU, which keeps the N * N * Do tanh evaluations.  Backward, per 16 pairs: the same pre-activations
// again, then dW += dpre^T p (rows = outputs, k = pairs: the accumulators of the first product ARE the left operand) into Do * D / 64
// accumulators per lane that live for the whole block, and dp^T = W^T dpre^T after one trip of the dpre tile through LDS (the only
// transposition); dP goes to HBM for gat_dx_kernel as before.  Blocks = scl_gat_score_nblocks(N) per graph, nodes i dealt out evenly,
// so the partial-sum layout the callers reduce is unchanged.
template <int D>
__device__ __forceinline__ void gat_stage_x(float* xs, const float* __restrict__ xb, int N) {      // [N + 16][D + 1], rows >= N zero
    for (int e = threadIdx.x; e < (N + 16) * D; e += GAT_PAIRS) { const int r = e / D, d = e - r * D; xs[r * (D + 1) + d] = r < N ? xb[e] : 0.f; }
}

// VAR: graphs of different sizes in one batch (scoring).  Utterance b has nodes[b] <= Nmax nodes, the first n1s[b] of the first type; x keeps
// the padded batch's strides ([B, Nmax, D], rows >= nodes[b] are not read), s is written as the utterance's own [nodes[b]][nodes[b]]
// matrix at the start of its Nmax * Nmax block.  Everything that differs per utterance is uniform in a workgroup.
template <int D, int Do, bool VAR = false>
__global__ __launch_bounds__(GAT_PAIRS, 1) void gat_score_fwd_mfma_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                         const float* __restrict__ bias, const float* __restrict__ a,
                                                                         float* __restrict__ s, int Nmax, int n1, const int* __restrict__ nodes = nullptr,
                                                                         const int* __restrict__ n1s = nullptr) {
    constexpr int NS = D / 4, NOB = Do / 16, XP = D + 1;
    extern __shared__ float sm[];
    float* xs = sm;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    int N = Nmax;
    if (VAR) {
        N = nodes[b]; N = N < 1 ? 1 : (N > Nmax ? Nmax : N);
        n1 = n1s ? n1s[b] : N; n1 = n1 < 0 ? 0 : (n1 > N ? N : n1);
        const int ipb_ = (N + (int)gridDim.x - 1) / (int)gridDim.x;
        if ((int)blockIdx.x * ipb_ >= N) return;      // a block wholly beyond the utterance's nodes: the whole workgroup leaves before any barrier
    }
    gat_stage_x<D>(xs, x + (int64_t)b * Nmax * D, N);
    float wr[NOB][NS], bo[NOB], av[3][NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
        const int o = 16 * ob + li;
        bo[ob] = bias[o];
#pragma unroll
        for (int t = 0; t < 3; ++t) av[t][ob] = a[t * Do + o];
#pragma unroll
        for (int k = 0; k < NS; ++k) wr[ob][k] = W[(size_t)o * D + 4 * k + g];
    }
    __syncthreads();
    const int nblk = gridDim.x, ipb = (N + nblk - 1) / nblk;
    const int i0 = blockIdx.x * ipb, i1 = min(N, i0 + ipb), njb = (N + 15) / 16;
    for (int u = wave; u < (i1 - i0) * njb; u += GAT_PAIRS / 64) {
        const int i = i0 + u / njb, j0 = (u % njb) * 16;
        f32x4 acc[NOB];
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const float pv = xs[i * XP + 4 * k + g] * xs[(j0 + li) * XP + 4 * k + g];
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) acc[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, wr[ob][k], acc[ob], 0, 0, 0);
        }
        float sc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
            const int ty = gat_type(i, j < N ? j : 0, n1);
            float v = 0.f;
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) v += gat_tanh(acc[ob][r] + bo[ob]) * (ty == 0 ? av[0][ob] : (ty == 1 ? av[1][ob] : av[2][ob]));
            sc[r] = lanes16_sum(v);
        }
        if (li == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int j = j0 + 4 * g + r; if (j < N) s[(int64_t)b * Nmax * Nmax + (int64_t)i * N + j] = sc[r]; }
        }
    }
}

// VAR (training on zero-padded batches): the backward of the VAR forward above.  N is the batch's Nmax - the strides of x and of the
// utterance's blocks of ds and dP - and the utterance's own N_b = nodes[b] and n1_b = n1s[b] replace N and n1 below: ds comes in the
// forward's ragged layout (the own [N_b][N_b] at the start of the Nmax * Nmax block, row stride N_b), dP is written in the same layout, and
// x rows and ds entries beyond the own graph are never read.  A block wholly beyond the utterance's nodes writes its row of `part` as zeros
// (the caller sums every row) and leaves before any barrier; all of this is uniform in a workgroup.
template <int D, int Do, bool VAR = false>
__global__ __launch_bounds__(GAT_PAIRS, 1) void gat_score_bwd_mfma_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                         const float* __restrict__ bias, const float* __restrict__ a,
                                                                         const float* __restrict__ ds, float* __restrict__ dP,
                                                                         float* __restrict__ part, int N, int n1, const int* __restrict__ nodes = nullptr,
                                                                         const int* __restrict__ n1s = nullptr) {
    constexpr int NS = D / 4, NOB = Do / 16, NDB = D / 16, NSO = Do / 4, XP = D + 1, TP = Do + 1;
    extern __shared__ float sm[];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const float* xb = x + (int64_t)b * N * D;                     // the padded batch's strides (VAR: N is still Nmax here)
    const float* dsb = ds + (int64_t)b * N * N;
    float* dPb = dP + (int64_t)b * N * N * D;
    if (VAR) {
        const int Nmax = N;
        N = nodes[b]; N = N < 1 ? 1 : (N > Nmax ? Nmax : N);
        n1 = n1s ? n1s[b] : N; n1 = n1 < 0 ? 0 : (n1 > N ? N : n1);
        const int ipb_ = (N + (int)gridDim.x - 1) / (int)gridDim.x;
        if ((int)blockIdx.x * ipb_ >= N) {
            float* pz = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ((size_t)Do * D + 4 * Do);
            for (int e = tid; e < Do * D + 4 * Do; e += GAT_PAIRS) pz[e] = 0.f;
            return;
        }
    }
    float* xs = sm;                                        // [N + 16][XP]
    float* Tw = sm + (N + 16) * XP + wave * 16 * TP;       // this wave's dpre tile [16 pairs][TP]
    float* red = sm + (N + 16) * XP + 4 * 16 * TP;         // [4 waves][4 * Do]: db | da0 | da1 | da2
    gat_stage_x<D>(xs, xb, N);
    float wr[NOB][NS], wt[NDB][NSO], bo[NOB], av[3][NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
        const int o = 16 * ob + li;
        bo[ob] = bias[o];
#pragma unroll
        for (int t = 0; t < 3; ++t) av[t][ob] = a[t * Do + o];
#pragma unroll
        for (int k = 0; k < NS; ++k) wr[ob][k] = W[(size_t)o * D + 4 * k + g];
    }
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int k = 0; k < NSO; ++k) wt[db][k] = W[(size_t)(4 * k + g) * D + 16 * db + li];      // W^T: row d = 16 db + li, k <-> o = 4 k + g
    f32x4 dwa[NOB][NDB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int db = 0; db < NDB; ++db) dwa[ob][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs[NOB], das[3][NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) { dbs[ob] = 0.f; das[0][ob] = 0.f; das[1][ob] = 0.f; das[2][ob] = 0.f; }
    __syncthreads();
    const int nblk = gridDim.x, ipb = (N + nblk - 1) / nblk;
    const int i0 = blockIdx.x * ipb, i1 = min(N, i0 + ipb), njb = (N + 15) / 16;
    for (int u = wave; u < (i1 - i0) * njb; u += GAT_PAIRS / 64) {
        const int i = i0 + u / njb, j0 = (u % njb) * 16;
        f32x4 acc[NOB];
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const float pv = xs[i * XP + 4 * k + g] * xs[(j0 + li) * XP + 4 * k + g];
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) acc[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, wr[ob][k], acc[ob], 0, 0, 0);
        }
        // this lane: outputs o = 16 ob + li of the pairs (i, j0 + 4 g + r)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
            const float gd = j < N ? dsb[(int64_t)i * N + j] : 0.f;
            const int ty = gat_type(i, j < N ? j : 0, n1);
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) {
                const float h = gat_tanh(acc[ob][r] + bo[ob]);
                const float at = ty == 0 ? av[0][ob] : (ty == 1 ? av[1][ob] : av[2][ob]);
                const float gh = gd * h;
                das[0][ob] += ty == 0 ? gh : 0.f; das[1][ob] += ty == 1 ? gh : 0.f; das[2][ob] += ty == 2 ? gh : 0.f;
                const float dpre = gd * at * (1.0f - h * h);
                dbs[ob] += dpre;
                acc[ob][r] = dpre;
                Tw[(4 * g + r) * TP + 16 * ob + li] = dpre;
            }
        }
        // dW[o][d] += sum_pairs dpre[pair][o] p[pair][d]:  rows = o, k = pairs (k index g <-> pair 4 g + r), columns = d
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const float pv = xs[i * XP + 16 * db + li] * xs[(j0 + 4 * g + r) * XP + 16 * db + li];
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob) dwa[ob][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[ob][r], pv, dwa[ob][db], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the tile's writes are this wave's own: in order, complete before the reads below
        // dp^T[d][pair] = sum_o W[o][d] dpre[pair][o]:  rows = d, k = o, columns = pairs (j0 + li)
        f32x4 dpa[NDB];
#pragma unroll
        for (int db = 0; db < NDB; ++db) dpa[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NSO; ++k) {
            const float tv = Tw[li * TP + 4 * k + g];
#pragma unroll
            for (int db = 0; db < NDB; ++db) dpa[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[db][k], tv, dpa[db], 0, 0, 0);
        }
        if (j0 + li < N) {
            float* out = dPb + ((int64_t)i * N + j0 + li) * D;
#pragma unroll
            for (int db = 0; db < NDB; ++db) *reinterpret_cast<f32x4*>(out + 16 * db + 4 * g) = dpa[db];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the reads are done before the next unit overwrites the tile
    }
    // ---- block partials: dW from the accumulators (rows o = 16 ob + 4 g + r', column d = 16 db + li), four waves summed through LDS in order
    float* pb = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ((size_t)Do * D + 4 * Do);
    __syncthreads();
    float* wsum = sm;                                      // [Do * D] (x is no longer needed)
    for (int w4 = 0; w4 < 4; ++w4) {
        if (wave == w4) {
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
                for (int db = 0; db < NDB; ++db)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int idx = (16 * ob + 4 * g + r) * D + 16 * db + li;
                        wsum[idx] = (w4 == 0 ? 0.f : wsum[idx]) + dwa[ob][db][r];
                    }
        }
        __syncthreads();
    }
    for (int e = tid; e < Do * D; e += GAT_PAIRS) pb[e] = wsum[e];
    __syncthreads();      // small graphs: the sums' staging area below may overlap wsum
    // db / da: sum over the four lane groups g (they hold different pairs of the same output), then over the waves
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
        float v[4] = {dbs[ob], das[0][ob], das[1][ob], das[2][ob]};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] += __shfl_xor(v[q], 16, 64);
            v[q] += __shfl_xor(v[q], 32, 64);
            if (g == 0) red[wave * 4 * Do + q * Do + 16 * ob + li] = v[q];
        }
    }
    __syncthreads();
    for (int e = tid; e < 4 * Do; e += GAT_PAIRS) pb[(size_t)Do * D + e] = (red[e] + red[4 * Do + e]) + (red[8 * Do + e] + red[12 * Do + e]);
}

// ---- tiled matrix-core forms (N > GAT_MAXN) -----------------------------------------------------------------------------------------------
// The same arithmetic per unit (one node i x 16 nodes j), but the LDS no longer holds the graph: a block owns ipb <= GAT_IPB consecutive
// nodes i, keeps their rows of x for its whole life, and walks j in tiles of GAT_JT rows staged one after another into the same buffer
// (two barriers per tile; a tile is (i1 - i0) * 8 units of ~64 MFMAs for a 32 KB load, so the re-staging is a few percent).  Rows of a tile
// at or beyond N are zero and their pairs are masked as before.  The pair type comes from the global i and j, so n1 may fall anywhere in
// any tile.  Units are dealt to the waves in a fixed order and the block partials are summed as in the whole-graph kernel: deterministic.
template <int D>
__device__ __forceinline__ void gat_stage_rows(float* xs, const float* __restrict__ xb, int r0, int rows, int N) {      // [rows][D + 1] <- x rows r0 .., rows >= N zero
    for (int e = threadIdx.x; e < rows * D; e += GAT_PAIRS) {
        const int r = e / D, d = e - r * D;
        xs[r * (D + 1) + d] = r0 + r < N ? xb[(int64_t)(r0 + r) * D + d] : 0.f;
    }
}

// VAR (scoring): graphs of different sizes in one batch, as the whole-graph VAR kernel above.  N is the batch's Nmax (x [B, Nmax, D], the
// grid ceil(Nmax / GAT_IPB) blocks of GAT_IPB rows each); the utterance's own N_b = nodes[b] and n1_b = n1s[b] replace N and n1 everywhere
// below: the tile loop ends at N_b, the pair type is the utterance's own, s is its own [N_b][N_b] matrix at the start of its Nmax * Nmax
// block.  A block whose first row is at or beyond N_b leaves before the first barrier; all of this is uniform in a workgroup.  A pair's
// arithmetic does not depend on which block owns its row, so the bits are those of the utterance scored alone by the fixed form.
template <int D, int Do, bool VAR = false>
__global__ __launch_bounds__(GAT_PAIRS, 1) void gat_score_fwd_tiled_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                          const float* __restrict__ bias, const float* __restrict__ a,
                                                                          float* __restrict__ s, int N, int n1, const int* __restrict__ nodes = nullptr,
                                                                          const int* __restrict__ n1s = nullptr) {
    constexpr int NS = D / 4, NOB = Do / 16, XP = D + 1;
    extern __shared__ float sm[];
    float* xi = sm;                      // [GAT_IPB][XP]: the block's own rows
    float* xj = sm + GAT_IPB * XP;       // [GAT_JT][XP]: the current tile of rows j
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const float* xb = x + (int64_t)b * N * D;      // the padded batch's stride (VAR: N is still Nmax here)
    float* sb = s + (int64_t)b * N * N;
    int ipb = GAT_IPB;
    if (VAR) {
        const int Nmax = N;
        N = nodes[b]; N = N < 1 ? 1 : (N > Nmax ? Nmax : N);
        n1 = n1s ? n1s[b] : N; n1 = n1 < 0 ? 0 : (n1 > N ? N : n1);
        if ((int)blockIdx.x * GAT_IPB >= N) return;
    } else {
        const int nblk = gridDim.x;
        ipb = (N + nblk - 1) / nblk;      // <= GAT_IPB (scl_gat_score_nblocks)
    }
    const int i0 = blockIdx.x * ipb, i1 = min(N, i0 + ipb);
    gat_stage_rows<D>(xi, xb, i0, GAT_IPB, N);
    float wr[NOB][NS], bo[NOB], av[3][NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
        const int o = 16 * ob + li;
        bo[ob] = bias[o];
#pragma unroll
        for (int t = 0; t < 3; ++t) av[t][ob] = a[t * Do + o];
#pragma unroll
        for (int k = 0; k < NS; ++k) wr[ob][k] = W[(size_t)o * D + 4 * k + g];
    }
    for (int t0 = 0; t0 < N; t0 += GAT_JT) {
        __syncthreads();      // the previous tile's readers are done
        gat_stage_rows<D>(xj, xb, t0, GAT_JT, N);
        __syncthreads();
        const int njb = (min(N - t0, GAT_JT) + 15) / 16;
        for (int u = wave; u < (i1 - i0) * njb; u += GAT_PAIRS / 64) {
            const int il = u / njb, jl = (u % njb) * 16, i = i0 + il, j0 = t0 + jl;
            f32x4 acc[NOB];
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) acc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const float pv = xi[il * XP + 4 * k + g] * xj[(jl + li) * XP + 4 * k + g];
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob) acc[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, wr[ob][k], acc[ob], 0, 0, 0);
            }
            float sc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 4 * g + r;
                const int ty = gat_type(i, j < N ? j : 0, n1);
                float v = 0.f;
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob) v += gat_tanh(acc[ob][r] + bo[ob]) * (ty == 0 ? av[0][ob] : (ty == 1 ? av[1][ob] : av[2][ob]));
                sc[r] = lanes16_sum(v);
            }
            if (li == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { const int j = j0 + 4 * g + r; if (j < N) sb[(int64_t)i * N + j] = sc[r]; }
            }
        }
    }
}

// VAR: as gat_score_bwd_mfma_kernel's, on the tiled forward's partition (GAT_IPB rows per block, the tile loop ends at N_b).
template <int D, int Do, bool VAR = false>
__global__ __launch_bounds__(GAT_PAIRS, 1) void gat_score_bwd_tiled_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                          const float* __restrict__ bias, const float* __restrict__ a,
                                                                          const float* __restrict__ ds, float* __restrict__ dP,
                                                                          float* __restrict__ part, int N, int n1, const int* __restrict__ nodes = nullptr,
                                                                          const int* __restrict__ n1s = nullptr) {
    constexpr int NS = D / 4, NOB = Do / 16, NDB = D / 16, NSO = Do / 4, XP = D + 1, TP = Do + 1, XROWS = GAT_IPB + GAT_JT;
    extern __shared__ float sm[];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    float* xi = sm;                                        // [GAT_IPB][XP]
    float* xj = sm + GAT_IPB * XP;                         // [GAT_JT][XP]
    float* Tw = sm + XROWS * XP + wave * 16 * TP;          // this wave's dpre tile [16 pairs][TP]
    float* red = sm + XROWS * XP + 4 * 16 * TP;            // [4 waves][4 * Do]: db | da0 | da1 | da2
    const float* xb = x + (int64_t)b * N * D;                     // the padded batch's strides (VAR: N is still Nmax here)
    const float* dsb = ds + (int64_t)b * N * N;
    float* dPb = dP + (int64_t)b * N * N * D;
    int ipb = GAT_IPB;
    if (VAR) {
        const int Nmax = N;
        N = nodes[b]; N = N < 1 ? 1 : (N > Nmax ? Nmax : N);
        n1 = n1s ? n1s[b] : N; n1 = n1 < 0 ? 0 : (n1 > N ? N : n1);
        if ((int)blockIdx.x * GAT_IPB >= N) {
            float* pz = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ((size_t)Do * D + 4 * Do);
            for (int e = tid; e < Do * D + 4 * Do; e += GAT_PAIRS) pz[e] = 0.f;
            return;
        }
    } else {
        const int nblk = gridDim.x;
        ipb = (N + nblk - 1) / nblk;      // <= GAT_IPB (scl_gat_score_nblocks)
    }
    const int i0 = blockIdx.x * ipb, i1 = min(N, i0 + ipb);
    gat_stage_rows<D>(xi, xb, i0, GAT_IPB, N);
    float wr[NOB][NS], wt[NDB][NSO], bo[NOB], av[3][NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
        const int o = 16 * ob + li;
        bo[ob] = bias[o];
#pragma unroll
        for (int t = 0; t < 3; ++t) av[t][ob] = a[t * Do + o];
#pragma unroll
        for (int k = 0; k < NS; ++k) wr[ob][k] = W[(size_t)o * D + 4 * k + g];
    }
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int k = 0; k < NSO; ++k) wt[db][k] = W[(size_t)(4 * k + g) * D + 16 * db + li];      // W^T: row d = 16 db + li, k <-> o = 4 k + g
    f32x4 dwa[NOB][NDB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int db = 0; db < NDB; ++db) dwa[ob][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs[NOB], das[3][NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) { dbs[ob] = 0.f; das[0][ob] = 0.f; das[1][ob] = 0.f; das[2][ob] = 0.f; }
    for (int t0 = 0; t0 < N; t0 += GAT_JT) {
        __syncthreads();      // the previous tile's readers are done
        gat_stage_rows<D>(xj, xb, t0, GAT_JT, N);
        __syncthreads();
        const int njb = (min(N - t0, GAT_JT) + 15) / 16;
        for (int u = wave; u < (i1 - i0) * njb; u += GAT_PAIRS / 64) {
            const int il = u / njb, jl = (u % njb) * 16, i = i0 + il, j0 = t0 + jl;
            f32x4 acc[NOB];
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) acc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const float pv = xi[il * XP + 4 * k + g] * xj[(jl + li) * XP + 4 * k + g];
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob) acc[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, wr[ob][k], acc[ob], 0, 0, 0);
            }
            // this lane: outputs o = 16 ob + li of the pairs (i, j0 + 4 g + r)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 4 * g + r;
                const float gd = j < N ? dsb[(int64_t)i * N + j] : 0.f;
                const int ty = gat_type(i, j < N ? j : 0, n1);
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob) {
                    const float h = gat_tanh(acc[ob][r] + bo[ob]);
                    const float at = ty == 0 ? av[0][ob] : (ty == 1 ? av[1][ob] : av[2][ob]);
                    const float gh = gd * h;
                    das[0][ob] += ty == 0 ? gh : 0.f; das[1][ob] += ty == 1 ? gh : 0.f; das[2][ob] += ty == 2 ? gh : 0.f;
                    const float dpre = gd * at * (1.0f - h * h);
                    dbs[ob] += dpre;
                    acc[ob][r] = dpre;
                    Tw[(4 * g + r) * TP + 16 * ob + li] = dpre;
                }
            }
            // dW[o][d] += sum_pairs dpre[pair][o] p[pair][d]:  rows = o, k = pairs (k index g <-> pair 4 g + r), columns = d
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    const float pv = xi[il * XP + 16 * db + li] * xj[(jl + 4 * g + r) * XP + 16 * db + li];
#pragma unroll
                    for (int ob = 0; ob < NOB; ++ob) dwa[ob][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[ob][r], pv, dwa[ob][db], 0, 0, 0);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the tile's writes are this wave's own: in order, complete before the reads below
            // dp^T[d][pair] = sum_o W[o][d] dpre[pair][o]:  rows = d, k = o, columns = pairs (j0 + li)
            f32x4 dpa[NDB];
#pragma unroll
            for (int db = 0; db < NDB; ++db) dpa[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NSO; ++k) {
                const float tv = Tw[li * TP + 4 * k + g];
#pragma unroll
                for (int db = 0; db < NDB; ++db) dpa[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[db][k], tv, dpa[db], 0, 0, 0);
            }
            if (j0 + li < N) {
                float* out = dPb + ((int64_t)i * N + j0 + li) * D;
#pragma unroll
                for (int db = 0; db < NDB; ++db) *reinterpret_cast<f32x4*>(out + 16 * db + 4 * g) = dpa[db];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the reads are done before the next unit overwrites the tile
        }
    }
    // ---- block partials, as in gat_score_bwd_mfma_kernel: dW through LDS wave by wave in order, then db / da
    float* pb = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ((size_t)Do * D + 4 * Do);
    __syncthreads();
    float* wsum = sm;                                      // [Do * D] <= XROWS * XP (x is no longer needed); does not reach red
    for (int w4 = 0; w4 < 4; ++w4) {
        if (wave == w4) {
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
                for (int db = 0; db < NDB; ++db)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int idx = (16 * ob + 4 * g + r) * D + 16 * db + li;
                        wsum[idx] = (w4 == 0 ? 0.f : wsum[idx]) + dwa[ob][db][r];
                    }
        }
        __syncthreads();
    }
    for (int e = tid; e < Do * D; e += GAT_PAIRS) pb[e] = wsum[e];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
        float v[4] = {dbs[ob], das[0][ob], das[1][ob], das[2][ob]};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] += __shfl_xor(v[q], 16, 64);
            v[q] += __shfl_xor(v[q], 32, 64);
            if (g == 0) red[wave * 4 * Do + q * Do + 16 * ob + li] = v[q];
        }
    }
    __syncthreads();
    for (int e = tid; e < 4 * Do; e += GAT_PAIRS) pb[(size_t)Do * D + e] = (red[e] + red[4 * Do + e]) + (red[8 * Do + e] + red[12 * Do + e]);
}

// Masked soft-max and aggregation in one pass (scoring): out[b][i][:] = sum_{j < N_b} softmax_j(s[b][i][j] / temp) * x[b][j][:] for the rows
// i < N_b, what F.softmax(s / temp, -1) followed by att @ x computes, without the [N][N] attention matrix in HBM.  s is read once, in the
// layout scl_gat_score_fwd_var writes (the utterance's own [N_b][N_b] matrix at the start of its Nmax * Nmax block); x is [B, Nmax, D].
// A block owns AGG_IPB = 16 rows i and walks j in tiles of AGG_JT = 64: the tile's scores become p = exp(s / temp - m) against a running row
// maximum m (the running sum and the accumulators are rescaled by exp(m_old - m_new) when it moves), p and the x tile wait in LDS, and wave w
// adds P [16 x 64] * x [64 x 16 columns w] on the f32 matrix core.  LDS is fixed: 16 x 65 + 64 x (D + 16) floats, 24.5 KB at D = 64.  Scores
// and x rows at and beyond N_b are never read (p = 0 and x = 0 are selected).  Rows i >= N_b of out are WRITTEN AS ZEROS.  ONE = true: a
// single score row per utterance (s [B, Nmax], out [B, D]): the master node's softmax(am, dim = -2)^T x.  The tile and row partition is
// fixed, so an utterance's bits do not depend on the batch it sits in.
constexpr int AGG_IPB = 16, AGG_JT = 64, AGG_PS = AGG_JT + 1;

__device__ __forceinline__ float lanes16_max_x(float v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float lanes16_sum_x(float v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int D, bool ONE>
__global__ __launch_bounds__(256) void gat_softmax_agg_kernel(const float* __restrict__ s, const float* __restrict__ x, const int* __restrict__ nodes,
                                                              float* __restrict__ out, int Nmax, float temp) {
    constexpr int NOB = D / 16, XS = D + 16;
    __shared__ float ps[AGG_IPB * AGG_PS];      // p of the tile [row][j]
    __shared__ float xs[AGG_JT * XS];           // x rows of the tile
    __shared__ float rs[2 * AGG_IPB];           // per row: this tile's rescale factor | at the end the running sum
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    int N = nodes[b]; N = N < 1 ? 1 : (N > Nmax ? Nmax : N);
    const int rows = ONE ? 1 : N, rows_max = ONE ? 1 : Nmax;
    const int i0 = blockIdx.x * AGG_IPB;
    float* ob_ = out + (int64_t)b * rows_max * D;
    if (i0 >= rows) {      // a block wholly beyond the utterance's rows: zeros, and out before any barrier (uniform in the workgroup)
        for (int e = tid; e < AGG_IPB * D; e += 256) { const int r = i0 + e / D; if (r < rows_max) ob_[(int64_t)r * D + (e % D)] = 0.f; }
        return;
    }
    const float* sb = s + (int64_t)b * (ONE ? Nmax : (int64_t)Nmax * Nmax);
    const float* xb = x + (int64_t)b * Nmax * D;
    const int row = tid >> 4, c = tid & 15, gi = i0 + row;      // the soft-max stage: 16 threads per row, 4 scores each
    const bool own = gi < rows;
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < N; t0 += AGG_JT) {
        float v[4], tmax = -INFINITY;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = t0 + c + 16 * q;
            v[q] = (own && j < N) ? sb[(int64_t)gi * N + j] / temp : -INFINITY;
            tmax = fmaxf(tmax, v[q]);
        }
        tmax = lanes16_max_x(tmax);
        const float m_new = fmaxf(m_run, tmax);
        const float sc = (m_new == -INFINITY) ? 0.f : expf(m_run - m_new);      // rows beyond the utterance keep p = 0, sc = 0
        float psum = 0.f;
        __syncthreads();      // the previous tile's readers are done
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float p = v[q] == -INFINITY ? 0.f : expf(v[q] - m_new);
            ps[row * AGG_PS + c + 16 * q] = p;
            psum += p;
        }
        l_run = l_run * sc + lanes16_sum_x(psum);
        m_run = m_new;
        if (c == 0) rs[row] = sc;
        for (int e = tid; e < AGG_JT * D; e += 256) {
            const int r = e / D, d = e - r * D;
            xs[r * XS + d] = t0 + r < N ? xb[(int64_t)(t0 + r) * D + d] : 0.f;
        }
        __syncthreads();
        if (wave < NOB) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] *= rs[4 * g + r];
#pragma unroll
            for (int kk = 0; kk < AGG_JT / 4; ++kk)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ps[li * AGG_PS + 4 * kk + g], xs[(4 * kk + g) * XS + 16 * wave + li], acc, 0, 0, 0);
        }
    }
    __syncthreads();
    if (c == 0) rs[AGG_IPB + row] = l_run;
    __syncthreads();
    if (wave < NOB) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * g + r;
            if (i < rows) ob_[(int64_t)i * D + 16 * wave + li] = acc[r] / rs[AGG_IPB + 4 * g + r];
            else if (i < rows_max) ob_[(int64_t)i * D + 16 * wave + li] = 0.f;
        }
    }
}

// Backward of the masked soft-max + aggregation (training on zero-padded batches).  With P = softmax_j(s / temp) over the own nodes,
//   dP[i][j] = dout[i] . x[j],   ds[i][j] = P[i][j] (dP[i][j] - sum_j' P[i][j'] dP[i][j']) / temp,   dx[j] = sum_i P[i][j] dout[i].
// P is recomputed from s by streaming; no [N][N] matrix but ds itself reaches HBM.  Two kernels, no atomics, fixed LDS (21 KB / 22 KB at D = 64):
//   rows  a block owns AGB_IPB = 16 rows i and walks j in tiles of AGB_JT = 64 twice.  First walk: the running row maximum m, the sum l and
//         r = sum_j p dP, rescaled together when m moves (the forward's scheme); m and l go to `stats` [B][rows][2].  Second walk: ds, written
//         in the ragged layout of s (entries beyond the own [N_b][N_b] are not written).
//   cols  a block owns 16 nodes j and walks i in tiles of 64 in order: p = exp(s / temp - m_i) / l_i from `stats`, dx[j] += p dout[i]; the rows
//         j >= N_b of dx [B, Nmax, D] are written as zeros.
// Neither reads s, x or dout beyond the own graph (0 is selected).  The row / tile partition is fixed and starts at 0 in every utterance, so
// an utterance's ds and dx do not depend on the batch it sits in.  ONE: the master node's single score row (s, ds [B, Nmax]; dout [B, D]).
constexpr int AGB_IPB = 16, AGB_JT = 64;

template <int D, bool ONE>
__global__ __launch_bounds__(256) void gat_softmax_agg_bwd_rows_kernel(const float* __restrict__ s, const float* __restrict__ x, const int* __restrict__ nodes,
                                                                       const float* __restrict__ dout, float* __restrict__ ds, float* __restrict__ stats,
                                                                       int Nmax, float temp) {
    constexpr int XS = D + 1;
    __shared__ float xs[AGB_JT * XS];       // x rows of the tile
    __shared__ float dos[AGB_IPB * XS];     // the block's rows of dout
    const int b = blockIdx.y, tid = threadIdx.x;
    int N = nodes[b]; N = N < 1 ? 1 : (N > Nmax ? Nmax : N);
    const int rows = ONE ? 1 : N, rows_max = ONE ? 1 : Nmax;
    const int i0 = blockIdx.x * AGB_IPB;
    if (i0 >= rows) return;      // a block wholly beyond the utterance's rows has nothing to write: out before any barrier (uniform in the workgroup)
    const float* sb = s + (int64_t)b * (ONE ? Nmax : (int64_t)Nmax * Nmax);
    float* dsb = ds + (int64_t)b * (ONE ? Nmax : (int64_t)Nmax * Nmax);
    const float* xb = x + (int64_t)b * Nmax * D;
    const float* dob = dout + (int64_t)b * rows_max * D;
    const int row = tid >> 4, c = tid & 15, gi = i0 + row;      // 16 threads per row, 4 pairs of a tile each
    const bool own = gi < rows;
    for (int e = tid; e < AGB_IPB * D; e += 256) {
        const int r = e / D, d = e - r * D;
        dos[r * XS + d] = i0 + r < rows ? dob[(int64_t)(i0 + r) * D + d] : 0.f;
    }
    float m_run = -INFINITY, l_run = 0.f, r_run = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        for (int t0 = 0; t0 < N; t0 += AGB_JT) {
            __syncthreads();      // the previous tile's readers are done
            for (int e = tid; e < AGB_JT * D; e += 256) {
                const int r = e / D, d = e - r * D;
                xs[r * XS + d] = t0 + r < N ? xb[(int64_t)(t0 + r) * D + d] : 0.f;
            }
            __syncthreads();
            float v[4], dp[4], tmax = -INFINITY;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int jl = c + 16 * q, j = t0 + jl;
                const bool ok = own && j < N;
                v[q] = ok ? sb[(int64_t)gi * N + j] / temp : -INFINITY;
                float acc = 0.f;
                for (int d = 0; d < D; ++d) acc += dos[row * XS + d] * xs[jl * XS + d];
                dp[q] = acc;
                tmax = fmaxf(tmax, v[q]);
            }
            if (pass == 0) {
                tmax = lanes16_max_x(tmax);
                const float m_new = fmaxf(m_run, tmax);
                const float sc = (m_new == -INFINITY) ? 0.f : expf(m_run - m_new);
                float psum = 0.f, prs = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float p = v[q] == -INFINITY ? 0.f : expf(v[q] - m_new);
                    psum += p; prs += p * dp[q];
                }
                l_run = l_run * sc + lanes16_sum_x(psum);
                r_run = r_run * sc + lanes16_sum_x(prs);
                m_run = m_new;
            } else if (own) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = t0 + c + 16 * q;
                    if (j < N) dsb[(int64_t)gi * N + j] = expf(v[q] - m_run) / l_run * (dp[q] - r_run) / temp;
                }
            }
        }
        if (pass == 0 && own) {      // l_run >= 1: the row's maximum contributes exp(0)
            r_run /= l_run;
            if (c == 0) { float* st = stats + ((int64_t)b * rows_max + gi) * 2; st[0] = m_run; st[1] = l_run; }
        }
    }
}

template <int D, bool ONE>
__global__ __launch_bounds__(256) void gat_softmax_agg_bwd_cols_kernel(const float* __restrict__ s, const int* __restrict__ nodes, const float* __restrict__ dout,
                                                                       const float* __restrict__ stats, float* __restrict__ dx, int Nmax, float temp) {
    constexpr int XS = D + 1, PS = 17, ND = D / 16;
    __shared__ float ps[AGB_JT * PS];       // p of the tile [row i][node j]
    __shared__ float dos[AGB_JT * XS];      // dout rows of the tile
    const int b = blockIdx.y, tid = threadIdx.x;
    int N = nodes[b]; N = N < 1 ? 1 : (N > Nmax ? Nmax : N);
    const int rows = ONE ? 1 : N, rows_max = ONE ? 1 : Nmax;
    const int j0 = blockIdx.x * 16;
    float* dxb = dx + (int64_t)b * Nmax * D;
    if (j0 >= N) {      // nodes wholly beyond the utterance's: zeros, and out before any barrier (uniform in the workgroup)
        for (int e = tid; e < 16 * D; e += 256) { const int j = j0 + e / D; if (j < Nmax) dxb[(int64_t)j * D + (e % D)] = 0.f; }
        return;
    }
    const float* sb = s + (int64_t)b * (ONE ? Nmax : (int64_t)Nmax * Nmax);
    const float* dob = dout + (int64_t)b * rows_max * D;
    const float* st = stats + (int64_t)b * rows_max * 2;
    const int jr = tid >> 4, dg = tid & 15;      // this thread: node j0 + jr, features dg + 16 k
    float acc[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) acc[k] = 0.f;
    for (int t0 = 0; t0 < rows; t0 += AGB_JT) {
        __syncthreads();      // the previous tile's readers are done
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q, il = e >> 4, jl = e & 15, i = t0 + il, j = j0 + jl;
            float p = 0.f;
            if (i < rows && j < N) p = expf(sb[(int64_t)i * N + j] / temp - st[2 * i]) / st[2 * i + 1];
            ps[il * PS + jl] = p;
        }
        for (int e = tid; e < AGB_JT * D; e += 256) {
            const int r = e / D, d = e - r * D;
            dos[r * XS + d] = t0 + r < rows ? dob[(int64_t)(t0 + r) * D + d] : 0.f;
        }
        __syncthreads();
        for (int il = 0; il < AGB_JT; ++il) {
            const float pv = ps[il * PS + jr];
#pragma unroll
            for (int k = 0; k < ND; ++k) acc[k] += pv * dos[il * XS + dg + 16 * k];
        }
    }
    const int j = j0 + jr;
    if (j < Nmax) {
#pragma unroll
        for (int k = 0; k < ND; ++k) dxb[(int64_t)j * D + dg + 16 * k] = j < N ? acc[k] : 0.f;
    }
}

template <int D, int Do>
constexpr size_t gat_tiled_lds(bool bwd) {      // independent of N: 35 KB forward, 56 KB backward at (64, 64)
    size_t f = (size_t)(GAT_IPB + GAT_JT) * (D + 1);
    if (bwd) f += 4 * 16 * (Do + 1) + 16 * Do;
    return f * sizeof(float);
}
static_assert(gat_tiled_lds<64, 64>(true) <= 64 * 1024, "the tiled forms stay under the default dynamic-LDS limit");

template <int D, int Do>
size_t gat_mfma_lds(int N, bool bwd) {
    size_t f = (size_t)(N + 16) * (D + 1);
    if (bwd) { f += 4 * 16 * (Do + 1) + 16 * Do; if (f < (size_t)Do * D) f = (size_t)Do * D; }
    return f * sizeof(float);
}

}  // namespace

// Up to GAT_MAXN nodes: one block per 256 pairs, as the whole-graph kernels always had.  Beyond: one block per GAT_IPB nodes i (the tiled
// forms), so the partial-sum buffer grows with N, not with N * N.
extern "C" int scl_gat_score_nblocks(int N) {
    return N <= GAT_MAXN ? (N * N + GAT_PAIRS - 1) / GAT_PAIRS : (N + GAT_IPB - 1) / GAT_IPB;
}

namespace {
bool gat_is_mfma(int D, int Do) { return (D == 64 && (Do == 64 || Do == 32)) || (D == 32 && Do == 32); }
}  // namespace

extern "C" int scl_gat_score_fwd(const float* x, const float* W, const float* bias, const float* a, float* s, int B, int N, int D, int Do,
                                 int n1, void* stream) {
    SCL_REQUIRE(x && W && bias && a && s && B > 0, "gat_score_fwd: null pointer");
    SCL_REQUIRE((D == 64 || D == 32) && Do >= 1 && Do <= 64 && N >= 1 && (N <= GAT_MAXN || gat_is_mfma(D, Do)) && n1 >= 0 && n1 <= N,
                "gat_score_fwd: need D in {32, 64}, Do <= 64, N <= 128 (D=%d Do=%d N=%d)", D, Do, N);
    SCL_REQUIRE(N <= GAT_CAP, "gat_score_fwd: at most %d nodes per graph (N=%d)", GAT_CAP, N);
    dim3 grid(scl_gat_score_nblocks(N), B), block(GAT_PAIRS);
    hipStream_t st = (hipStream_t)stream;
    if (N > GAT_MAXN) {
#define GAT_FWD_TILED(DD, OO) hipLaunchKernelGGL((gat_score_fwd_tiled_kernel<DD, OO>), grid, block, (gat_tiled_lds<DD, OO>(false)), st, x, W, bias, a, s, N, n1)
        if (D == 64 && Do == 64) GAT_FWD_TILED(64, 64);
        else if (D == 64 && Do == 32) GAT_FWD_TILED(64, 32);
        else GAT_FWD_TILED(32, 32);
#undef GAT_FWD_TILED
        return scl_check_launch("scl_gat_score_fwd");
    }
#define GAT_FWD_MFMA(DD, OO) hipLaunchKernelGGL((gat_score_fwd_mfma_kernel<DD, OO>), grid, block, (gat_mfma_lds<DD, OO>(N, false)), st, x, W, bias, a, s, N, n1, (const int*)nullptr, (const int*)nullptr)
    if (D == 64 && Do == 64) { GAT_FWD_MFMA(64, 64); return scl_check_launch("scl_gat_score_fwd"); }
    if (D == 64 && Do == 32) { GAT_FWD_MFMA(64, 32); return scl_check_launch("scl_gat_score_fwd"); }
    if (D == 32 && Do == 32) { GAT_FWD_MFMA(32, 32); return scl_check_launch("scl_gat_score_fwd"); }
#undef GAT_FWD_MFMA
    if (D == 64) {
        const size_t lds = GatSmem<64>::floats(Do, N) * sizeof(float);
        hipLaunchKernelGGL((gat_score_fwd_kernel<64>), grid, block, lds, st, x, W, bias, a, s, N, Do, n1);
    } else {
        const size_t lds = GatSmem<32>::floats(Do, N) * sizeof(float);
        hipLaunchKernelGGL((gat_score_fwd_kernel<32>), grid, block, lds, st, x, W, bias, a, s, N, Do, n1);
    }
    return scl_check_launch("scl_gat_score_fwd");
}

extern "C" int scl_gat_score_fwd_var(const float* x, const float* W, const float* bias, const float* a, float* s, const int32_t* nodes, const int32_t* n1,
                                     int B, int Nmax, int D, int Do, void* stream) {
    SCL_REQUIRE(x && W && bias && a && s && nodes && B > 0, "scl_gat_score_fwd_var: null pointer");
    SCL_REQUIRE(((D == 64 && (Do == 64 || Do == 32)) || (D == 32 && Do == 32)) && Nmax >= 1 && Nmax <= GAT_CAP,
                "scl_gat_score_fwd_var: the matrix-core forms only: (D, Do) in {(64, 64), (64, 32), (32, 32)}, Nmax <= %d (D=%d Do=%d Nmax=%d)", GAT_CAP, D,
                Do, Nmax);
    SCL_REQUIRE(Nmax <= GAT_MAXN || n1, "scl_gat_score_fwd_var: above %d nodes the tiled form reads both tables: n1 == NULL is refused (a homogeneous "
                "layer passes nodes as n1) (Nmax=%d)", GAT_MAXN, Nmax);
    dim3 grid(scl_gat_score_nblocks(Nmax), B), block(GAT_PAIRS);
    hipStream_t st = (hipStream_t)stream;
    if (Nmax > GAT_MAXN) {    // the tiled form: ceil(Nmax / GAT_IPB) blocks of GAT_IPB rows per utterance (what scl_gat_score_nblocks gives above GAT_MAXN)
#define GAT_FWD_TILED_VAR(DD, OO) hipLaunchKernelGGL((gat_score_fwd_tiled_kernel<DD, OO, true>), grid, block, (gat_tiled_lds<DD, OO>(false)), st, x, W, bias, a, s, Nmax, 0, nodes, n1)
        if (D == 64 && Do == 64) GAT_FWD_TILED_VAR(64, 64);
        else if (D == 64 && Do == 32) GAT_FWD_TILED_VAR(64, 32);
        else GAT_FWD_TILED_VAR(32, 32);
#undef GAT_FWD_TILED_VAR
        return scl_check_launch("scl_gat_score_fwd_var");
    }
#define GAT_FWD_VAR(DD, OO) hipLaunchKernelGGL((gat_score_fwd_mfma_kernel<DD, OO, true>), grid, block, (gat_mfma_lds<DD, OO>(Nmax, false)), st, x, W, bias, a, s, Nmax, 0, nodes, n1)
    if (D == 64 && Do == 64) GAT_FWD_VAR(64, 64);
    else if (D == 64 && Do == 32) GAT_FWD_VAR(64, 32);
    else GAT_FWD_VAR(32, 32);
#undef GAT_FWD_VAR
    return scl_check_launch("scl_gat_score_fwd_var");
}

// out[b][i][:] = sum_{j < nodes[b]} softmax_j(s[b][i][j] / temp) x[b][j][:], s as scl_gat_score_fwd_var lays it out, x [B, Nmax, D], out [B, Nmax, D]
// with its rows i >= nodes[b] written as zeros.  one_row: s [B, Nmax] holds a single score row per utterance and out is [B, D].
extern "C" int scl_gat_softmax_agg_var(const float* s, const float* x, const int32_t* nodes, float* out, int B, int Nmax, int D, int one_row, float temp,
                                       void* stream) {
    SCL_REQUIRE(s && x && nodes && out && B > 0 && B <= 65535, "scl_gat_softmax_agg_var: null pointer or batch beyond 65535");
    SCL_REQUIRE((D == 64 || D == 32) && Nmax >= 1 && Nmax <= GAT_CAP && temp > 0.f, "scl_gat_softmax_agg_var: need D in {32, 64}, 1 <= Nmax <= %d, temp > 0 (D=%d Nmax=%d)",
                GAT_CAP, D, Nmax);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(one_row ? 1 : (Nmax + AGG_IPB - 1) / AGG_IPB, B), block(256);
    if (D == 64 && one_row) hipLaunchKernelGGL((gat_softmax_agg_kernel<64, true>), grid, block, 0, st, s, x, nodes, out, Nmax, temp);
    else if (D == 64) hipLaunchKernelGGL((gat_softmax_agg_kernel<64, false>), grid, block, 0, st, s, x, nodes, out, Nmax, temp);
    else if (one_row) hipLaunchKernelGGL((gat_softmax_agg_kernel<32, true>), grid, block, 0, st, s, x, nodes, out, Nmax, temp);
    else hipLaunchKernelGGL((gat_softmax_agg_kernel<32, false>), grid, block, 0, st, s, x, nodes, out, Nmax, temp);
    return scl_check_launch("scl_gat_softmax_agg_var");
}

// dP: f32 [B, N*N, D] scratch; part: f32 [B * nblocks(N)][Do*D + 4*Do] partial sums (dW | dbias | da11 | da22 | da12), to be
// summed over their first dimension by the caller (scl_colreduce_*); dx: f32 [B, N, D]
extern "C" int scl_gat_score_bwd(const float* x, const float* W, const float* bias, const float* a, const float* ds, float* dP, float* part,
                                 float* dx, int B, int N, int D, int Do, int n1, void* stream) {
    SCL_REQUIRE(x && W && bias && a && ds && dP && part && dx && B > 0, "gat_score_bwd: null pointer");
    SCL_REQUIRE((D == 64 || D == 32) && Do >= 1 && Do <= 64 && N >= 1 && (N <= GAT_MAXN || gat_is_mfma(D, Do)) && n1 >= 0 && n1 <= N,
                "gat_score_bwd: need D in {32, 64}, Do <= 64, N <= 128 (D=%d Do=%d N=%d)", D, Do, N);
    SCL_REQUIRE(N <= GAT_CAP, "gat_score_bwd: at most %d nodes per graph (N=%d)", GAT_CAP, N);
    dim3 grid(scl_gat_score_nblocks(N), B), block(GAT_PAIRS);
    hipStream_t st = (hipStream_t)stream;
    if (N > GAT_MAXN) {
#define GAT_BWD_TILED(DD, OO)                                                                                                                         \
    do {                                                                                                                                               \
        hipLaunchKernelGGL((gat_score_bwd_tiled_kernel<DD, OO>), grid, block, (gat_tiled_lds<DD, OO>(true)), st, x, W, bias, a, ds, dP, part, N, n1);    \
        hipLaunchKernelGGL((gat_dx_kernel<DD>), dim3(N, B), dim3(4 * DD), 0, st, dP, x, dx, N);                                                        \
    } while (0)
        if (D == 64 && Do == 64) GAT_BWD_TILED(64, 64);
        else if (D == 64 && Do == 32) GAT_BWD_TILED(64, 32);
        else GAT_BWD_TILED(32, 32);
#undef GAT_BWD_TILED
        return scl_check_launch("scl_gat_score_bwd");
    }
    static bool attr_set = false;
    if (!attr_set) {
        hipFuncSetAttribute((const void*)gat_score_bwd_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipFuncSetAttribute((const void*)gat_score_bwd_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
#define GAT_BWD_MFMA(DD, OO)                                                                                                                             \
    do {                                                                                                                                                  \
        hipLaunchKernelGGL((gat_score_bwd_mfma_kernel<DD, OO>), grid, block, (gat_mfma_lds<DD, OO>(N, true)), st, x, W, bias, a, ds, dP, part, N, n1);      \
        hipLaunchKernelGGL((gat_dx_kernel<DD>), dim3(N, B), dim3(4 * DD), 0, st, dP, x, dx, N);                                                           \
        return scl_check_launch("scl_gat_score_bwd");                                                                                                   \
    } while (0)
    if (D == 64 && Do == 64) GAT_BWD_MFMA(64, 64);
    if (D == 64 && Do == 32) GAT_BWD_MFMA(64, 32);
    if (D == 32 && Do == 32) GAT_BWD_MFMA(32, 32);
#undef GAT_BWD_MFMA
    if (D == 64) {
        const size_t lds = (((GatSmem<64>::floats(Do, N) + 3) & ~(size_t)3) + (size_t)GAT_PAIRS * GAT_DPS + 16 * Do) * sizeof(float) + 2 * GAT_PAIRS;
        SCL_REQUIRE(lds <= 160 * 1024, "gat_score_bwd: LDS tile too large");
        hipLaunchKernelGGL((gat_score_bwd_kernel<64>), grid, block, lds, st, x, W, bias, a, ds, dP, part, N, Do, n1);
        hipLaunchKernelGGL((gat_dx_kernel<64>), dim3(N, B), dim3(256), 0, st, dP, x, dx, N);
    } else {
        const size_t lds = (((GatSmem<32>::floats(Do, N) + 3) & ~(size_t)3) + (size_t)GAT_PAIRS * GAT_DPS + 16 * Do) * sizeof(float) + 2 * GAT_PAIRS;
        SCL_REQUIRE(lds <= 160 * 1024, "gat_score_bwd: LDS tile too large");
        hipLaunchKernelGGL((gat_score_bwd_kernel<32>), grid, block, lds, st, x, W, bias, a, ds, dP, part, N, Do, n1);
        hipLaunchKernelGGL((gat_dx_kernel<32>), dim3(N, B), dim3(128), 0, st, dP, x, dx, N);
    }
    return scl_check_launch("scl_gat_score_bwd");
}

// Backward of scl_gat_score_fwd_var: graphs of different sizes in one batch.  ds and dP in the forward's ragged layout (the utterance's own
// [N_b][N_b] (x D) matrix at the start of its Nmax * Nmax (x D) block), dx [B, Nmax, D] with its rows >= N_b written as zeros, part as
// scl_gat_score_bwd's with scl_gat_score_nblocks(Nmax) rows per utterance - the rows of blocks beyond N_b are zeros.
extern "C" int scl_gat_score_bwd_var(const float* x, const float* W, const float* bias, const float* a, const float* ds, float* dP, float* part,
                                     float* dx, const int32_t* nodes, const int32_t* n1, int B, int Nmax, int D, int Do, void* stream) {
    SCL_REQUIRE(x && W && bias && a && ds && dP && part && dx && nodes && B > 0 && B <= 65535, "scl_gat_score_bwd_var: null pointer or batch beyond 65535");
    SCL_REQUIRE(gat_is_mfma(D, Do) && Nmax >= 1 && Nmax <= GAT_CAP,
                "scl_gat_score_bwd_var: the matrix-core forms only: (D, Do) in {(64, 64), (64, 32), (32, 32)}, Nmax <= %d (D=%d Do=%d Nmax=%d)", GAT_CAP, D,
                Do, Nmax);
    SCL_REQUIRE(Nmax <= GAT_MAXN || n1, "scl_gat_score_bwd_var: above %d nodes the tiled form reads both tables: n1 == NULL is refused (a homogeneous "
                "layer passes nodes as n1) (Nmax=%d)", GAT_MAXN, Nmax);
    dim3 grid(scl_gat_score_nblocks(Nmax), B), block(GAT_PAIRS);
    hipStream_t st = (hipStream_t)stream;
#define GAT_BWD_VAR(KERNEL, LDS, DD, OO)                                                                                                  \
    do {                                                                                                                                   \
        hipLaunchKernelGGL((KERNEL<DD, OO, true>), grid, block, (LDS), st, x, W, bias, a, ds, dP, part, Nmax, 0, nodes, n1);                 \
        hipLaunchKernelGGL((gat_dx_kernel<DD, true>), dim3(Nmax, B), dim3(4 * DD), 0, st, dP, x, dx, Nmax, nodes);                         \
    } while (0)
    if (Nmax > GAT_MAXN) {
        if (D == 64 && Do == 64) GAT_BWD_VAR(gat_score_bwd_tiled_kernel, (gat_tiled_lds<64, 64>(true)), 64, 64);
        else if (D == 64 && Do == 32) GAT_BWD_VAR(gat_score_bwd_tiled_kernel, (gat_tiled_lds<64, 32>(true)), 64, 32);
        else GAT_BWD_VAR(gat_score_bwd_tiled_kernel, (gat_tiled_lds<32, 32>(true)), 32, 32);
    } else {
        if (D == 64 && Do == 64) GAT_BWD_VAR(gat_score_bwd_mfma_kernel, (gat_mfma_lds<64, 64>(Nmax, true)), 64, 64);
        else if (D == 64 && Do == 32) GAT_BWD_VAR(gat_score_bwd_mfma_kernel, (gat_mfma_lds<64, 32>(Nmax, true)), 64, 32);
        else GAT_BWD_VAR(gat_score_bwd_mfma_kernel, (gat_mfma_lds<32, 32>(Nmax, true)), 32, 32);
    }
#undef GAT_BWD_VAR
    return scl_check_launch("scl_gat_score_bwd_var");
}

// Backward of scl_gat_softmax_agg_var: ds in the layout of s (the utterance's own [N_b][N_b] at the start of its Nmax * Nmax block; entries beyond
// are not written), dx [B, Nmax, D] with its rows >= N_b written as zeros.  stats: f32 [B, Nmax, 2] scratch (one_row: [B, 2]), the rows' soft-max
// maximum and sum handed from the first kernel to the second.  one_row: s, ds [B, Nmax] and dout [B, D].
extern "C" int scl_gat_softmax_agg_var_bwd(const float* s, const float* x, const int32_t* nodes, const float* dout, float* ds, float* dx, float* stats,
                                           int B, int Nmax, int D, int one_row, float temp, void* stream) {
    SCL_REQUIRE(s && x && nodes && dout && ds && dx && stats && B > 0 && B <= 65535, "scl_gat_softmax_agg_var_bwd: null pointer or batch beyond 65535");
    SCL_REQUIRE((D == 64 || D == 32) && Nmax >= 1 && Nmax <= GAT_CAP && temp > 0.f,
                "scl_gat_softmax_agg_var_bwd: need D in {32, 64}, 1 <= Nmax <= %d, temp > 0 (D=%d Nmax=%d)", GAT_CAP, D, Nmax);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid_r(one_row ? 1 : (Nmax + AGB_IPB - 1) / AGB_IPB, B), grid_c((Nmax + 15) / 16, B), block(256);
#define AGG_BWD(DD, ONE)                                                                                                                    \
    do {                                                                                                                                     \
        hipLaunchKernelGGL((gat_softmax_agg_bwd_rows_kernel<DD, ONE>), grid_r, block, 0, st, s, x, nodes, dout, ds, stats, Nmax, temp);       \
        hipLaunchKernelGGL((gat_softmax_agg_bwd_cols_kernel<DD, ONE>), grid_c, block, 0, st, s, nodes, dout, (const float*)stats, dx, Nmax, temp); \
    } while (0)
    if (D == 64 && one_row) AGG_BWD(64, true);
    else if (D == 64) AGG_BWD(64, false);
    else if (one_row) AGG_BWD(32, true);
    else AGG_BWD(32, false);
#undef AGG_BWD
    return scl_check_launch("scl_gat_softmax_agg_var_bwd");
}
