// Multi-view attention fusion head of MVP (model.py:28-48, 57-71), the consumer of the graph
// view: shared LayerNorm(384) on the three view embeddings, Q/K/V projection
// (three bias-free Linear(384 -> 12 x 384), one GEMM), attention over the 3 view tokens per head,
// Conv2d(12, 12, 3) + ReLU over the (head, token, feature) cube, MLP 4584 -> 1024 -> 11, and
// BCEWithLogitsLoss (main.py:91).  The GEMMs go through mvml_gemm_f32x3; the non-GEMM kernels and
// their backward are in three files:
//   * fusion_attn.hip: LayerNorm rows (one wave per row), token attention, plain and with the
//     Q.K product folded (one wave per (molecule, head) / per molecule; the 3x3 scores are nine
//     wave dot products, the rows stream once), BCE-with-logits;
//   * fusion_conv.hip: the 3x3 convolution on the matrix cores, one workgroup per run of
//     molecules with the (12, 3, 384) cube staged in LDS, and the fixed-order sum of the
//     per-workgroup weight-gradient partials (deterministic, no atomics);
//   * fusion_attn_conv.hip: attention and convolution fused, the cube never leaving LDS.
// This header holds what more than one of them uses: the masked column accesses, the 3 x 3 score
// arithmetic the fused and unfused kernels must do in one order, the convolution's sizes and
// staging, and the choice of a kernel instance by width.
// 384 above is the default head width D = hidden_feats[-1]; the token-attention and fused kernels
// take any multiple of 4 in [16, 384] (templates over <kMask, kV>, see col_ld below), the
// LayerNorm rows up to 512 and the convolution any 3 <= W <= 384.
//
// Everything device-side here sits in the unnamed namespace and is forced inline, so no kernel
// symbol comes from this header: each kernel is defined in exactly one of the three files.
#pragma once
#include "common.h"

namespace mvml {

// g_weight[1296] and g_bias[12] of a Conv2d backward: the fixed-order sums over the nblk partial
// rows (kConvPart floats each) its workgroups wrote (fusion_conv.hip); the last launch's status
int sum_conv_partials(int nblk, const float* part, float* g_weight, float* g_bias, hipStream_t st);

namespace {

// Attention over the NT = 3 view tokens of one molecule, per head (model.py:62-68):
//   q/k/v of token t = QKV row 3b+t, columns [h*dk | HD + h*dk | 2HD + h*dk] (dk wide)
//   s_ij = <q_i, k_j> * scale;  p = softmax_j(s);  att[b][h][i] = sum_j p_ij v_j
constexpr int NT = 3;
constexpr int kDkVpl = 6;  // dk <= 384 = 6 x 64: lane l covers the columns l + 64 i, i < 6

// Every token-attention and fused kernel is a template over <kMask, kV>, kV = ceil(dk / 64) the 64-column groups a
// lane holds.  <false, 6> is the dk = 384 instance: six full groups, no column test anywhere
// (the helpers fold away).  <true, kV> takes any dk in (64 (kV - 1), 64 kV]: the groups
// i < kV - 1 are full, and only the last one is masked.  A column c >= dk of that group is read
// from the always-in-range address of column dk - 1 and replaced by an exact 0 by a select (so
// it adds nothing to a dot product or a maximum, and no load is branched around), and is never
// stored.
template <bool kMask, int kV>
__device__ __forceinline__ bool col_ok(int lane, int i, int dk) {
  return (kMask && i == kV - 1) ? lane + 64 * i < dk : true;
}
// column lane + 64 i of the dk-wide row that starts at base[off]
template <bool kMask, int kV, typename Off>
__device__ __forceinline__ float col_ld(const float* base, Off off, int lane, int i, int dk) {
  if (kMask && i == kV - 1) {
    const float v = base[off + min(lane + 64 * i, dk - 1)];
    return lane + 64 * i < dk ? v : 0.f;
  }
  return base[off + lane + 64 * i];
}
// the same with the column c = lane + 64 i formed by the caller (base[off + c])
template <bool kMask, int kV, typename Off>
__device__ __forceinline__ float col_ldc(const float* base, Off off, int c, int i, int dk) {
  if (kMask && i == kV - 1) {
    const float v = base[off + min(c, dk - 1)];
    return c < dk ? v : 0.f;
  }
  return base[off + c];
}

// Softmax backward of one head's 3 x 3 scores: g_p_ac = <g_a, v_c> (wave sums), then
// g_s_ac = p_ac (g_p_ac - sum_c' p_ac' g_p_ac') scale, with every product and sum explicit (no
// contraction left to the compiler), so the fused and unfused kernels agree bit for bit.
template <int kV>
__device__ __forceinline__ void fold_grad_scores(const float (&g)[NT][kV],
                                                 const float (&v)[NT][kV],
                                                 const float (&p)[NT][NT], float scale,
                                                 float (&gs)[NT][NT]) {
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    float gp[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      float sc = 0.f;
#pragma unroll
      for (int i = 0; i < kV; ++i) sc = fmaf(g[a][i], v[c][i], sc);
      gp[c] = wave_sum(sc);
    }
    const float dot = fmaf(p[a][2], gp[2], fmaf(p[a][1], gp[1], __fmul_rn(p[a][0], gp[0])));
#pragma unroll
    for (int c = 0; c < NT; ++c) gs[a][c] = __fmul_rn(__fmul_rn(p[a][c], __fsub_rn(gp[c], dot)), scale);
  }
}

// softmax(scale * <q_a, k_c>) over c for the 3 x 3 scores of one head (token_attn_fold_fwd's order)
template <int kV>
__device__ __forceinline__ void fold_scores(const float (&q)[NT][kV], const float (&k)[NT][kV],
                                            float scale, float (&p)[NT][NT]) {
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      float sc = 0.f;
#pragma unroll
      for (int i = 0; i < kV; ++i) sc = fmaf(q[a][i], k[c][i], sc);
      p[a][c] = wave_sum(sc) * scale;
    }
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    const float m = fmaxf(p[a][0], fmaxf(p[a][1], p[a][2]));
    float z = 0.f;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      p[a][c] = expf(p[a][c] - m);
      z += p[a][c];
    }
#pragma unroll
    for (int c = 0; c < NT; ++c) p[a][c] /= z;
  }
}

// Conv2d(C, O, 3) over the (C, 3, W) cube of one molecule (model.py:27, 69): the kernel height
// equals the token count, so the output is (O, 1, W - 2); + bias, ReLU (model.py:27-28).
constexpr int kConvC = 12, kConvO = 12, kConvH = 3;
constexpr int kConvThreads = 384;
constexpr int kConvWg = kConvO * kConvC * kConvH * 3;  // 1296 weights
constexpr int kConvLd = 385;  // LDS row stride (W <= 384): rows land on different banks

// rows x W floats from global (row-contiguous) into LDS rows of stride kConvLd.  The aligned path
// issues all of a thread's loads (<= kStageIt float4: 36 rows x 384 / 384 threads = 9) before its
// first LDS store — one memory round trip per molecule instead of one per float4.
constexpr int kStageIt = 9;
__device__ __forceinline__ void conv_stage(float* dst, const float* __restrict__ src, int rows, int W,
                                           int tid) {
  const int w4 = W >> 2;
  if ((W & 3) == 0 && ((uintptr_t)src & 15) == 0 && rows * w4 <= kStageIt * kConvThreads) {
    float4 v[kStageIt];
#pragma unroll
    for (int it = 0; it < kStageIt; ++it) {
      const int i = tid + it * kConvThreads;
      if (i < rows * w4) {
        const int r = i / w4, c = (i - r * w4) * 4;
        v[it] = *reinterpret_cast<const float4*>(src + (int64_t)r * W + c);
      }
    }
#pragma unroll
    for (int it = 0; it < kStageIt; ++it) {
      const int i = tid + it * kConvThreads;
      if (i < rows * w4) {
        const int r = i / w4, c = (i - r * w4) * 4;
        float* d = dst + r * kConvLd + c;
        d[0] = v[it].x; d[1] = v[it].y; d[2] = v[it].z; d[3] = v[it].w;
      }
    }
  } else {
    for (int i = tid; i < rows * W; i += kConvThreads) dst[(i / W) * kConvLd + i % W] = src[i];
  }
}

// Per-workgroup partial row of the backward kernels: the 1296 weight-gradient sums (o, c, dy, dx),
// then kConvWg floats nothing writes or reads, then (at 2 * kConvWg) the 12 bias-gradient sums.
// The gap is kept: the row length and the bias offset are immediates of conv3_bwd2_kernel and of
// every attn_conv_bwd_kernel instance and set mvml_*_bwd_workspace_size, so closing it would
// change those kernels' code and the sizes callers allocate.
constexpr int kConvPart = 2 * kConvWg + kConvO;

typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int kConvNT = 7;                     // 16-column tiles of n (108 weights + bias)

// The head width the token-attention and fused kernels take: a multiple of 4 in [16, 384]
// (the GAT / Set2Set kernels upstream emit multiples of 4; 384 is the conv kernels' LDS row).
inline bool fuse_dk_ok(int dk) { return dk >= 16 && dk <= 64 * kDkVpl && dk % 4 == 0; }
#define MVML_DK_SET "dk must be a multiple of 4 in [16, 384]"

// Width -> kernel instance, the whole table: dk = 384 is the unmasked <false, 6>, every other
// width the masked <true, ceil(dk / 64)>.  fn(mask, kv) gets the pair as integral constants
// (kernel<mask.value, kv.value>) and launches; its result is returned.
template <typename Fn>
int by_width(int dk, Fn&& fn) {
  if (dk == 64 * kDkVpl) return fn(std::false_type{}, std::integral_constant<int, kDkVpl>{});
  return switch_const<1, 2, 3, 4, 5, 6>((int)ceil_div(dk, 64),
                                        [&](auto kv) { return fn(std::true_type{}, kv); });
}

}  // namespace
}  // namespace mvml
