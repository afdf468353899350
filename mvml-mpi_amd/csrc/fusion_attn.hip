// Fusion head, the row kernels (overview in fusion_common.h): LayerNorm rows, attention over the
// three view tokens with Q, K, V rows (token_attn_*) or with the Q.K product folded into the
// projection (token_attn_fold_*), BCE-with-logits, and their entry points.
#include "fusion_common.h"

namespace mvml {
namespace {

constexpr int kFuseMaxVpl = 8;  // LayerNorm rows up to 512 wide

// LayerNorm (torch.nn.LayerNorm, biased variance, eps inside the sqrt), one wave per row.
__global__ void __launch_bounds__(256)
layernorm_fwd_kernel(int64_t rows, int D, const float* __restrict__ x, int64_t ldx,
                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                     float* __restrict__ y, int64_t ldy, float* __restrict__ mean_out,
                     float* __restrict__ rstd_out) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  float v[kFuseMaxVpl];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kFuseMaxVpl; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < D ? x[r * ldx + c] : 0.f;
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < kFuseMaxVpl; ++i) {
    const int c = lane + 64 * i;
    const float d = c < D ? v[i] - mean : 0.f;
    q += d * d;
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < kFuseMaxVpl; ++i) {
    const int c = lane + 64 * i;
    if (c < D) y[r * ldy + c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
  }
  if (lane == 0) {
    mean_out[r] = mean;
    rstd_out[r] = rstd;
  }
}

// g_x = rstd * (g_xh - mean(g_xh) - xh * mean(g_xh * xh)), g_xh = g_y * gamma;
// gxh_out = g_y * xh (its column sums are dL/dgamma; column sums of g_y are dL/dbeta).
__global__ void __launch_bounds__(256)
layernorm_bwd_kernel(int64_t rows, int D, const float* __restrict__ x, int64_t ldx,
                     const float* __restrict__ gamma, const float* __restrict__ mean_in,
                     const float* __restrict__ rstd_in, const float* __restrict__ gy,
                     int64_t ldgy, float* __restrict__ gx, int64_t ldgx,
                     float* __restrict__ gyxh) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float mean = mean_in[r], rstd = rstd_in[r];
  float xh[kFuseMaxVpl], g[kFuseMaxVpl];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < kFuseMaxVpl; ++i) {
    const int c = lane + 64 * i;
    xh[i] = c < D ? (x[r * ldx + c] - mean) * rstd : 0.f;
    const float gyv = c < D ? gy[r * ldgy + c] : 0.f;
    g[i] = c < D ? gyv * gamma[c] : 0.f;
    if (c < D) gyxh[r * D + c] = gyv * xh[i];
    s1 += g[i];
    s2 += g[i] * xh[i];
  }
  const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
  for (int i = 0; i < kFuseMaxVpl; ++i) {
    const int c = lane + 64 * i;
    if (c < D) gx[r * ldgx + c] = rstd * (g[i] - m1 - xh[i] * m2);
  }
}

// Plain token attention, one wave per (molecule, head).  The scores and softmax below repeat
// fold_scores, and the store of the nine probabilities is written out in each forward kernel:
// calling a shared helper here compiles to a different instruction stream in every instance.
template <bool kMask, int kV>
__global__ void __launch_bounds__(256)
token_attn_fwd_kernel(int64_t B, int H, int dk, const float* __restrict__ qkv, int64_t ld,
                      float scale, float* __restrict__ att, float* __restrict__ P) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= B * H) return;
  const int64_t b = w / H;
  const int h = (int)(w % H);
  const int64_t HD = (int64_t)H * dk;
  float q[NT][kV], k[NT][kV], v[NT][kV];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float* row = qkv + (b * NT + t) * ld + (int64_t)h * dk;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      const int c = lane + 64 * i;
      q[t][i] = col_ldc<kMask, kV>(row, 0, c, i, dk);
      k[t][i] = col_ldc<kMask, kV>(row, HD, c, i, dk);
      v[t][i] = col_ldc<kMask, kV>(row, 2 * HD, c, i, dk);
    }
  }
  float p[NT][NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < kV; ++i) s = fmaf(q[a][i], k[c][i], s);
      p[a][c] = wave_sum(s) * scale;
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
  float* out = att + w * NT * dk;
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      float o = 0.f;
#pragma unroll
      for (int c = 0; c < NT; ++c) o = fmaf(p[a][c], v[c][i], o);
      if (col_ok<kMask, kV>(lane, i, dk)) out[a * dk + lane + 64 * i] = o;
    }
  if (lane < NT * NT) {
    float pv = p[0][0];
#pragma unroll
    for (int e = 1; e < NT * NT; ++e) pv = lane == e ? p[e / NT][e % NT] : pv;
    P[w * NT * NT + lane] = pv;
  }
}

// Backward of token_attn_fwd: g_v_j = sum_i p_ij g_i;  g_p_ij = <g_i, v_j>;
// g_s_ij = p_ij (g_p_ij - sum_j' p_ij' g_p_ij');  g_q_i = scale sum_j g_s_ij k_j;
// g_k_j = scale sum_i g_s_ij q_i.  gqkv has the layout of qkv.
template <bool kMask, int kV>
__global__ void __launch_bounds__(256)
token_attn_bwd_kernel(int64_t B, int H, int dk, const float* __restrict__ qkv, int64_t ld,
                      float scale, const float* __restrict__ P, const float* __restrict__ g_att,
                      float* __restrict__ gqkv, int64_t ldg) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= B * H) return;
  const int64_t b = w / H;
  const int h = (int)(w % H);
  const int64_t HD = (int64_t)H * dk;
  float p[NT][NT];
#pragma unroll
  for (int e = 0; e < NT * NT; ++e) p[e / NT][e % NT] = P[w * NT * NT + e];
  float g[NT][kV], v[NT][kV];
  const float* ga = g_att + w * NT * dk;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float* row = qkv + (b * NT + t) * ld + (int64_t)h * dk;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      const int c = lane + 64 * i;
      g[t][i] = col_ldc<kMask, kV>(ga, t * dk, c, i, dk);
      v[t][i] = col_ldc<kMask, kV>(row, 2 * HD, c, i, dk);
    }
  }
  float gs[NT][NT];
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    float gp[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < kV; ++i) s = fmaf(g[a][i], v[c][i], s);
      gp[c] = wave_sum(s);
    }
    const float dot = p[a][0] * gp[0] + p[a][1] * gp[1] + p[a][2] * gp[2];
#pragma unroll
    for (int c = 0; c < NT; ++c) gs[a][c] = p[a][c] * (gp[c] - dot) * scale;
  }
  // g_v (reuses v registers), then g_q, g_k from q, k
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    float* grow = gqkv + (b * NT + c) * ldg + (int64_t)h * dk;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      float o = 0.f;
#pragma unroll
      for (int a = 0; a < NT; ++a) o = fmaf(p[a][c], g[a][i], o);
      if (col_ok<kMask, kV>(lane, i, dk)) grow[2 * HD + lane + 64 * i] = o;
    }
  }
  float q[NT][kV], k[NT][kV];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float* row = qkv + (b * NT + t) * ld + (int64_t)h * dk;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      q[t][i] = col_ld<kMask, kV>(row, 0, lane, i, dk);
      k[t][i] = col_ld<kMask, kV>(row, HD, lane, i, dk);
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float* grow = gqkv + (b * NT + t) * ldg + (int64_t)h * dk;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      float oq = 0.f, ok = 0.f;
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        oq = fmaf(gs[t][c], k[c][i], oq);
        ok = fmaf(gs[c][t], q[c][i], ok);
      }
      if (col_ok<kMask, kV>(lane, i, dk)) {
        grow[lane + 64 * i] = oq;
        grow[HD + lane + 64 * i] = ok;
      }
    }
  }
}

// Folded Q.K (the QK^T of model.py:65-68 re-associated): s_ij = <q_i, k_j> = x_i W_q^T W_k x_j^T
// = <p_i, x_j> with p = x M_h, M_h = W_q,h^T W_k,h (D x D per head), so the product GEMM forms
// [P | V] = X [M_1 .. M_H | W_v^T] (2 H D columns instead of 3 H D) and the attention reads the
// LayerNorm rows x_j themselves as the keys of every head.  One wave per MOLECULE walks the
// heads in order: the three key rows are loaded once, and the backward sums the key gradient
// over the heads in registers (fixed order) into g_k = sum_h g_k,h, so the data-gradient GEMM
// also runs over 2 H D columns.
//   pv rows 3b+t = [p (H dk) | v (H dk)] (ld >= 2 H dk); x rows 3b+t (dk); att, P as above.
template <bool kMask, int kV>
__global__ void __launch_bounds__(256)
token_attn_fold_fwd_kernel(int64_t B, int H, int dk, const float* __restrict__ pv, int64_t ld,
                           const float* __restrict__ x, int64_t ldx, float scale,
                           float* __restrict__ att, float* __restrict__ P) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const int64_t HD = (int64_t)H * dk;
  float k[NT][kV];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < kV; ++i) k[t][i] = col_ld<kMask, kV>(x, (b * NT + t) * ldx, lane, i, dk);
  for (int h = 0; h < H; ++h) {
    float q[NT][kV], v[NT][kV];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float* row = pv + (b * NT + t) * ld + (int64_t)h * dk;
#pragma unroll
      for (int i = 0; i < kV; ++i) {
        q[t][i] = col_ld<kMask, kV>(row, 0, lane, i, dk);
        v[t][i] = col_ld<kMask, kV>(row, HD, lane, i, dk);
      }
    }
    float p[NT][NT];  // fold_scores written out (see token_attn_fwd_kernel)
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
    const int64_t w = b * H + h;
    float* out = att + w * NT * dk;
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int i = 0; i < kV; ++i) {
        float o = 0.f;
#pragma unroll
        for (int c = 0; c < NT; ++c) o = fmaf(p[a][c], v[c][i], o);
        if (col_ok<kMask, kV>(lane, i, dk)) out[a * dk + lane + 64 * i] = o;
      }
    if (lane < NT * NT) {
      float pvv = p[0][0];
#pragma unroll
      for (int e = 1; e < NT * NT; ++e) pvv = lane == e ? p[e / NT][e % NT] : pvv;
      P[w * NT * NT + lane] = pvv;
    }
  }
}

// Backward of token_attn_fold_fwd: g_v_j = sum_i p_ij g_i; g_s = p (g_p - <p, g_p>) scale;
// g_p_i = sum_j g_s_ij x_j; g_k_j = sum_h sum_i g_s_ij p_i (heads in order).
template <bool kMask, int kV>
__global__ void __launch_bounds__(256)
token_attn_fold_bwd_kernel(int64_t B, int H, int dk, const float* __restrict__ pv, int64_t ld,
                           const float* __restrict__ x, int64_t ldx, float scale,
                           const float* __restrict__ P, const float* __restrict__ g_att,
                           float* __restrict__ gpv, int64_t ldg, float* __restrict__ gk,
                           int64_t ldgk, uint32_t* __restrict__ gpv_amax) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  float gmx = 0.f;  // |max| of this lane's gpv stores (split-fp16 scale of the two GEMMs)
  const int64_t HD = (int64_t)H * dk;
  float k[NT][kV], gks[NT][kV];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      k[t][i] = col_ld<kMask, kV>(x, (b * NT + t) * ldx, lane, i, dk);
      gks[t][i] = 0.f;
    }
  for (int h = 0; h < H; ++h) {
    const int64_t w = b * H + h;
    float p[NT][NT];
#pragma unroll
    for (int e = 0; e < NT * NT; ++e) p[e / NT][e % NT] = P[w * NT * NT + e];
    float g[NT][kV], v[NT][kV];
    const float* ga = g_att + w * NT * dk;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float* row = pv + (b * NT + t) * ld + (int64_t)h * dk;
#pragma unroll
      for (int i = 0; i < kV; ++i) {
        g[t][i] = col_ld<kMask, kV>(ga, t * dk, lane, i, dk);
        v[t][i] = col_ld<kMask, kV>(row, HD, lane, i, dk);
      }
    }
    float gs[NT][NT];
    fold_grad_scores(g, v, p, scale, gs);
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      float* grow = gpv + (b * NT + c) * ldg + (int64_t)h * dk;
#pragma unroll
      for (int i = 0; i < kV; ++i) {
        float o = 0.f;
#pragma unroll
        for (int a = 0; a < NT; ++a) o = fmaf(p[a][c], g[a][i], o);
        if (col_ok<kMask, kV>(lane, i, dk)) grow[HD + lane + 64 * i] = o;
        gmx = fmaxf(gmx, fabsf(o));
      }
    }
    float q[NT][kV];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float* row = pv + (b * NT + t) * ld + (int64_t)h * dk;
#pragma unroll
      for (int i = 0; i < kV; ++i) q[t][i] = col_ld<kMask, kV>(row, 0, lane, i, dk);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float* grow = gpv + (b * NT + t) * ldg + (int64_t)h * dk;
#pragma unroll
      for (int i = 0; i < kV; ++i) {
        float oq = 0.f, ok = 0.f;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
          oq = fmaf(gs[t][c], k[c][i], oq);
          ok = fmaf(gs[c][t], q[c][i], ok);
        }
        if (col_ok<kMask, kV>(lane, i, dk)) grow[lane + 64 * i] = oq;
        gmx = fmaxf(gmx, fabsf(oq));
        gks[t][i] += ok;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < kV; ++i)
      if (col_ok<kMask, kV>(lane, i, dk)) gk[(b * NT + t) * ldgk + lane + 64 * i] = gks[t][i];
  if (gpv_amax) {  // one unsigned atomicMax of the float bits per wave (waves may exit early)
    gmx = wave_max(gmx);
    if (lane == 0) atomicMax(gpv_amax, __float_as_uint(gmx));
  }
}

// BCEWithLogitsLoss (mean over all B x C logits, main.py:91): per-element loss terms (summed by
// the caller) and dL/dz = (sigmoid(z) - y) / (B C).
__global__ void bce_logits_kernel(int64_t n, const float* __restrict__ z, const float* __restrict__ y,
                                  float* __restrict__ loss_terms, float* __restrict__ gz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float zi = z[i], yi = y[i];
  // max(z, 0) - z y + log(1 + exp(-|z|)): torch's stable form
  loss_terms[i] = fmaxf(zi, 0.f) - zi * yi + log1pf(expf(-fabsf(zi)));
  gz[i] = (1.f / (1.f + expf(-zi)) - yi) / (float)n;
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_layernorm_fwd(int64_t rows, int D, const float* x, int64_t ldx,
                                  const float* gamma, const float* beta, float eps, float* y,
                                  int64_t ldy, float* mean, float* rstd, void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && D > 0 && D <= 64 * kFuseMaxVpl && ldx >= D && ldy >= D,
               "layernorm_fwd: bad shape (D must be <= %d)", 64 * kFuseMaxVpl);
  if (rows == 0) return MVML_OK;
  MVML_REQUIRE(x && gamma && beta && y && mean && rstd, "layernorm_fwd: NULL pointer");
  layernorm_fwd_kernel<<<(unsigned)ceil_div(rows, 4), 256, 0, as_stream(stream)>>>(
      rows, D, x, ldx, gamma, beta, eps, y, ldy, mean, rstd);
  return check_launch("layernorm_fwd_kernel");
}

extern "C" int mvml_layernorm_bwd(int64_t rows, int D, const float* x, int64_t ldx,
                                  const float* gamma, const float* mean, const float* rstd,
                                  const float* g_y, int64_t ldgy, float* g_x, int64_t ldgx,
                                  float* g_y_xhat, void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && D > 0 && D <= 64 * kFuseMaxVpl && ldx >= D && ldgy >= D && ldgx >= D,
               "layernorm_bwd: bad shape");
  if (rows == 0) return MVML_OK;
  MVML_REQUIRE(x && gamma && mean && rstd && g_y && g_x && g_y_xhat, "layernorm_bwd: NULL pointer");
  layernorm_bwd_kernel<<<(unsigned)ceil_div(rows, 4), 256, 0, as_stream(stream)>>>(
      rows, D, x, ldx, gamma, mean, rstd, g_y, ldgy, g_x, ldgx, g_y_xhat);
  return check_launch("layernorm_bwd_kernel");
}

extern "C" int mvml_token_attn_fwd(int64_t B, int H, int dk, const float* qkv, int64_t ld,
                                   float scale, float* att, float* P, void* stream) {
  clear_error();
  MVML_REQUIRE(B >= 0 && H > 0 && fuse_dk_ok(dk) && ld >= 3 * (int64_t)H * dk,
               "token_attn_fwd: " MVML_DK_SET " and ld >= 3*H*dk");
  if (B == 0) return MVML_OK;
  MVML_REQUIRE(qkv && att && P, "token_attn_fwd: NULL pointer");
  return by_width(dk, [&](auto mask, auto kv) {
    token_attn_fwd_kernel<mask.value, kv.value>
        <<<(unsigned)ceil_div(B * H, 4), 256, 0, as_stream(stream)>>>(B, H, dk, qkv, ld, scale, att, P);
    return check_launch("token_attn_fwd_kernel");
  });
}

extern "C" int mvml_token_attn_bwd(int64_t B, int H, int dk, const float* qkv, int64_t ld,
                                   float scale, const float* P, const float* g_att,
                                   float* g_qkv, int64_t ldg, void* stream) {
  clear_error();
  MVML_REQUIRE(B >= 0 && H > 0 && fuse_dk_ok(dk) && ld >= 3 * (int64_t)H * dk &&
                   ldg >= 3 * (int64_t)H * dk,
               "token_attn_bwd: bad shape (" MVML_DK_SET ")");
  if (B == 0) return MVML_OK;
  MVML_REQUIRE(qkv && P && g_att && g_qkv, "token_attn_bwd: NULL pointer");
  return by_width(dk, [&](auto mask, auto kv) {
    token_attn_bwd_kernel<mask.value, kv.value><<<(unsigned)ceil_div(B * H, 4), 256, 0, as_stream(stream)>>>(
        B, H, dk, qkv, ld, scale, P, g_att, g_qkv, ldg);
    return check_launch("token_attn_bwd_kernel");
  });
}

extern "C" int mvml_token_attn_fold_fwd(int64_t B, int H, int dk, const float* pv, int64_t ld,
                                        const float* x, int64_t ldx, float scale, float* att,
                                        float* P, void* stream) {
  clear_error();
  MVML_REQUIRE(B >= 0 && H > 0 && fuse_dk_ok(dk) && ld >= 2 * (int64_t)H * dk && ldx >= dk,
               "token_attn_fold_fwd: " MVML_DK_SET ", ld >= 2*H*dk");
  if (B == 0) return MVML_OK;
  return by_width(dk, [&](auto mask, auto kv) {
    token_attn_fold_fwd_kernel<mask.value, kv.value><<<(unsigned)ceil_div(B, 4), 256, 0, as_stream(stream)>>>(
        B, H, dk, pv, ld, x, ldx, scale, att, P);
    return check_launch("token_attn_fold_fwd_kernel");
  });
}

extern "C" int mvml_token_attn_fold_bwd(int64_t B, int H, int dk, const float* pv, int64_t ld,
                                        const float* x, int64_t ldx, float scale, const float* P,
                                        const float* g_att, float* g_pv, int64_t ldg, float* g_k,
                                        int64_t ldgk, uint32_t* gpv_amax, void* stream) {
  clear_error();
  MVML_REQUIRE(B >= 0 && H > 0 && fuse_dk_ok(dk) && ld >= 2 * (int64_t)H * dk && ldx >= dk &&
                   ldg >= 2 * (int64_t)H * dk && ldgk >= dk,
               "token_attn_fold_bwd: bad shape (" MVML_DK_SET ")");
  if (B == 0) return MVML_OK;
  return by_width(dk, [&](auto mask, auto kv) {
    token_attn_fold_bwd_kernel<mask.value, kv.value><<<(unsigned)ceil_div(B, 4), 256, 0, as_stream(stream)>>>(
        B, H, dk, pv, ld, x, ldx, scale, P, g_att, g_pv, ldg, g_k, ldgk, gpv_amax);
    return check_launch("token_attn_fold_bwd_kernel");
  });
}

extern "C" int mvml_bce_logits(int64_t n, const float* z, const float* y, float* loss_terms,
                               float* g_z, void* stream) {
  clear_error();
  MVML_REQUIRE(n >= 0, "bce_logits: bad size");
  if (n == 0) return MVML_OK;
  MVML_REQUIRE(z && y && loss_terms && g_z, "bce_logits: NULL pointer");
  bce_logits_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, as_stream(stream)>>>(n, z, y, loss_terms, g_z);
  return check_launch("bce_logits_kernel");
}
