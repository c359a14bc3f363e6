// attn_wide.h — the launchers of attention_wide.hip and attention_f32_wide.hip: the streaming attention for head dims 72..128 (D % 8 == 0),
// all three row layouts in bf16 and the packed fp32 forward.  They are internal to the library (hidden, C++ linkage): the C ABI entries of
// attention_long.hip, attention_varlen.hip, attention_packed.hip and attention_f32.hip validate their arguments, then hand a head dim that
// scl_attn_wide_takes over to them.
#pragma once
#include <cstdint>

enum SclAttnRows { SCL_ROWS_FIXED = 0, SCL_ROWS_PADDED = 1, SCL_ROWS_PACKED = 2 };

// the head dims of the padded families DP = 96 (72..96) and DP = 128 (104..128)
inline bool scl_attn_wide_takes(int D) { return D > 64 && D <= 128 && D % 8 == 0; }
// the refusal of every streaming entry ("head dim 64" is what callers and tests match on)
#define SCL_ATTN_HEAD_DIMS "needs head dim 64, or 72..128 in steps of 8"

// lens: nullptr (fixed), klen[B] (padded) or row0[B + 1] (packed); Mq: the packed launch's row count, 0 otherwise; `who`: the entry's name
// for the launch check.  ws: the delta workspace of scl_attn_long_ws_bytes(B, T, H).
__attribute__((visibility("hidden"))) int scl_attn_wide_fwd(SclAttnRows rows, const char* who, const void* qkv, void* ctx, float* lse,
                                                            const int32_t* lens, int B, int T, int H, int D, int Mq, float scale, float drop_p,
                                                            uint32_t drop_seed, void* stream);
__attribute__((visibility("hidden"))) int scl_attn_wide_bwd(SclAttnRows rows, const char* who, const void* qkv, const void* ctx, const void* dctx,
                                                            const float* lse, const int32_t* lens, void* dqkv, void* ws, int B, int T, int H, int D,
                                                            int Mq, float scale, float drop_p, uint32_t drop_seed, void* stream);
// attention_f32_wide.hip: the fp32 pair-form forward over packed rows, with the arguments of scl_attn_fwd_packed_f32 (attention_f32.hip),
// which validates them first
__attribute__((visibility("hidden"))) int scl_attn_wide_fwd_f32(const float* qkv, float* ctx, const int32_t* row0, int B, int T, int H, int D,
                                                                int Mq, float scale, void* stream);
