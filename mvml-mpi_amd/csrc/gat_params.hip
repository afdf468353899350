// The parameter side of a GAT layer, around the aggregation (gat_agg_fwd.hip / gat_agg_bwd.hip;
// the projection row layout: gat_agg_common.h): the projection with its logits, the weight fold /
// unfold of the one-GEMM layout, dL/dattn_{l,r} and the head mean of an identity residual.
#include "common.h"
#include "wave_ops.h"

namespace mvml {
namespace {

// Logits: el[n,h] = <Z[n,h,:], attn_l[h,:]>, er likewise.  The projection GEMM's epilogue leaves
// per-W-column partial dots part[g][side][n]; this sums a head's F/32 blocks in order and
// writes the compact elr[n] = [el | er] (the softmax's gathers and the backward read it).
template <int H>
__global__ void __launch_bounds__(256)
gat_logits_finalize_kernel(int64_t N, int F, int W, const float* __restrict__ part,
                           float* __restrict__ elr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over N * 2H
  if (i >= N * 2 * H) return;
  const int64_t v = i % N;           // node-fastest: coalesced partial reads
  const int sh = (int)(i / N);        // side * H + h
  const int side = sh / H, h = sh % H;
  const int nbh = F / W;
  const float* p = part + ((int64_t)(h * nbh) * 2 + side) * N + v;  // [group][side][node]
  float acc = p[0];
  for (int b = 1; b < nbh; ++b) acc += p[(int64_t)b * 2 * N];
  elr[v * 2 * H + sh] = acc;
}
// ------------------------------------------------------------------ parameter-side helpers
// dL/dattn_l[h,f] = sum_n d el[n,h] * Z[n,h,f] (likewise attn_r with d er), summed directly over
// atoms as autograd does.  Stage 1: each thread owns one Z column over a chunk of atoms.
__global__ void attn_grad_partial_kernel(int64_t N, int H, int F, const float* __restrict__ Y,
                                         int64_t ldy, const float* __restrict__ gelr, int64_t ldgl,
                                         int64_t rows_per, float* __restrict__ part) {
  const int HF = H * F;
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= HF) return;
  const int h = col / F;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = min(N, r0 + rows_per);
  float sl[4] = {0.f, 0.f, 0.f, 0.f}, sr[4] = {0.f, 0.f, 0.f, 0.f};
  int64_t r = r0;
  for (; r + 4 <= r1; r += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float z = Y[(r + j) * ldy + col];
      const float* g = gelr + (r + j) * ldgl;
      sl[j] = fmaf(g[h], z, sl[j]);
      sr[j] = fmaf(g[H + h], z, sr[j]);
    }
  }
  for (; r < r1; ++r) {
    const float z = Y[r * ldy + col];
    const float* g = gelr + r * ldgl;
    sl[0] = fmaf(g[h], z, sl[0]);
    sr[0] = fmaf(g[H + h], z, sr[0]);
  }
  part[((int64_t)blockIdx.y * 2 + 0) * HF + col] = (sl[0] + sl[1]) + (sl[2] + sl[3]);
  part[((int64_t)blockIdx.y * 2 + 1) * HF + col] = (sr[0] + sr[1]) + (sr[2] + sr[3]);
}

__global__ void attn_grad_final_kernel(int HF, int S, const float* __restrict__ part,
                                       float* __restrict__ g_al, float* __restrict__ g_ar) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over 2*HF
  if (i >= 2 * HF) return;
  const int side = i / HF, col = i % HF;
  float s = 0.f;
  for (int z = 0; z < S; ++z) s += part[((int64_t)z * 2 + side) * HF + col];
  (side ? g_ar : g_al)[col] = s;
}

int attn_grad_splits(int64_t N, int HF) {
  const int64_t colblocks = ceil_div(HF, 256);
  int64_t s = ceil_div(2048, colblocks);
  s = std::min<int64_t>(s, ceil_div(N, 256));
  return (int)std::max<int64_t>(1, s);
}

// Wcat rows: [0,HF) fc.weight | [HF,HF+RW) res_fc.weight (RW = HF) or its head mean (RW = F) or
// nothing (mean_res == MVML_RES_NONE: RW = 0, res_w unused); columns Fin..ldw-1 are zero.
__global__ void fold_weights_kernel(const float* __restrict__ fc_w, const float* __restrict__ res_w,
                                    const float* __restrict__ attn_lr, int H, int F, int Fin,
                                    int ldw, int mean_res, float* __restrict__ Wcat) {
  const int HF = H * F;
  const int RW = mean_res == MVML_RES_NONE ? 0 : mean_res ? F : HF;
  const int64_t total = (int64_t)(HF + RW + (attn_lr ? 2 * H : 0)) * ldw;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(e / ldw), k = (int)(e % ldw);
    float v;
    if (k >= Fin) {
      v = 0.f;
    } else if (row < HF) {
      v = fc_w[(int64_t)row * Fin + k];
    } else if (row >= HF + RW) {  // A_l / A_r rows: sum_f attn[h, f] fc.weight[h F + f, k]
      const int side = (row - HF - RW) / H, h = (row - HF - RW) % H;
      const float* a = attn_lr + side * HF + h * F;
      float acc = 0.f;
      for (int f = 0; f < F; ++f) acc = fmaf(a[f], fc_w[(int64_t)(h * F + f) * Fin + k], acc);
      v = acc;
    } else {
      const int r = row - HF;
      if (mean_res) {
        float s = 0.f;
        for (int h = 0; h < H; ++h) s += res_w[(int64_t)(h * F + r) * Fin + k];
        v = s / (float)H;
      } else {
        v = res_w[(int64_t)r * Fin + k];
      }
    }
    Wcat[e] = v;
  }
}

// dL/dfc.weight = gWcat[0:HF] (+ attn_l[h,f] gWcat[C+h] + attn_r[h,f] gWcat[C+H+h]: the el / er
// paths, when the backward folded them into the GEMM);  dL/dres_fc.weight[hF+f] =
// gWcat[HF+hF+f] or gWcat[HF+f] / H.
__global__ void unfold_w_kernel(const float* __restrict__ gW, const float* __restrict__ attn_lr,
                                int H, int F, int Fin, int ldg, int mean_res,
                                float* __restrict__ g_fc, float* __restrict__ g_res) {
  const int HF = H * F;
  const int C = HF + (mean_res == MVML_RES_NONE ? 0 : mean_res ? F : HF);
  const int64_t total = (int64_t)HF * Fin;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(e / Fin), k = (int)(e % Fin);
    float gf = gW[(int64_t)row * ldg + k];
    if (attn_lr) {
      const int h = row / F;
      gf = fmaf(attn_lr[row], gW[(int64_t)(C + h) * ldg + k], gf);
      gf = fmaf(attn_lr[HF + row], gW[(int64_t)(C + H + h) * ldg + k], gf);
    }
    g_fc[e] = gf;
    if (mean_res == MVML_RES_NONE) continue;  // no residual rows: g_res is not written
    g_res[e] = mean_res ? gW[(int64_t)(HF + row % F) * ldg + k] / (float)H
                        : gW[(int64_t)(HF + row) * ldg + k];
  }
}

// Head mean of flattened rows (the identity residual of a head-mean layer) and its backward:
// one thread per (atom, f-float4); heads summed in order, then / H (torch mean(1)).
__global__ void __launch_bounds__(256)
head_mean_kernel(int64_t N, int H, int F, const float* __restrict__ X, int64_t ldx,
                 float* __restrict__ R, int64_t ldr) {
  const int nf4 = F / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * nf4) return;
  const int64_t n = i / nf4;
  const int c = 4 * (int)(i % nf4);
  float4 s = ld4(X + n * ldx + c);
  for (int h = 1; h < H; ++h) s = add4(s, ld4(X + n * ldx + h * F + c));
  const float hh = (float)H;
  st4(R + n * ldr + c, make_float4(s.x / hh, s.y / hh, s.z / hh, s.w / hh));
}

__global__ void __launch_bounds__(256)
head_mean_bwd_kernel(int64_t N, int H, int F, const float* __restrict__ gR, int64_t ldgr,
                     float* __restrict__ gX, int64_t ldgx) {
  const int nf4 = F / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * nf4) return;
  const int64_t n = i / nf4;
  const int c = 4 * (int)(i % nf4);
  const float4 g = ld4(gR + n * ldgr + c);
  const float hh = (float)H;
  const float4 v = make_float4(g.x / hh, g.y / hh, g.z / hh, g.w / hh);
  for (int h = 0; h < H; ++h) st4(gX + n * ldgx + h * F + c, v);
}

int check_head_mean(int64_t N, int H, int F, const void* a, int64_t lda, int64_t wa, const void* b,
                    int64_t ldb, int64_t wb, const char* who) {
  MVML_REQUIRE(N >= 0 && H > 0 && F > 0 && F % 4 == 0, "%s: H > 0 and F a positive multiple of 4", who);
  MVML_REQUIRE(lda >= wa && ldb >= wb && lda % 4 == 0 && ldb % 4 == 0 && aligned16(a) && aligned16(b),
               "%s: rows must be 16-byte aligned (pointers and row strides)", who);
  return MVML_OK;
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_head_mean_f32(int64_t N, int H, int F, const float* X, int64_t ldx, float* R,
                                  int64_t ldr, void* stream) {
  clear_error();
  int rc = check_head_mean(N, H, F, X, ldx, (int64_t)H * F, R, ldr, F, "head_mean");
  if (rc || N == 0) return rc;
  head_mean_kernel<<<(unsigned)ceil_div(N * (F / 4), 256), 256, 0, as_stream(stream)>>>(N, H, F, X, ldx, R, ldr);
  return check_launch("head_mean_kernel");
}

extern "C" int mvml_head_mean_bwd_f32(int64_t N, int H, int F, const float* gR, int64_t ldgr, float* gX,
                                      int64_t ldgx, void* stream) {
  clear_error();
  int rc = check_head_mean(N, H, F, gR, ldgr, F, gX, ldgx, (int64_t)H * F, "head_mean_bwd");
  if (rc || N == 0) return rc;
  head_mean_bwd_kernel<<<(unsigned)ceil_div(N * (F / 4), 256), 256, 0, as_stream(stream)>>>(N, H, F, gR, ldgr, gX,
                                                                                         ldgx);
  return check_launch("head_mean_bwd_kernel");
}

extern "C" int mvml_gat_proj_cols(int H, int F, int mean_residual) {
  return H * F + (mean_residual ? F : H * F);
}

extern "C" int mvml_gat_proj_cols_res(int H, int F, int res) {
  return res == MVML_RES_NONE ? H * F : mvml_gat_proj_cols(H, F, res == MVML_RES_MEAN);
}

extern "C" size_t mvml_gat_proj_fwd_workspace_size(int64_t num_nodes, int H, int F) {
  // logit partials, then 256 B for the split-fp16 operand maxima
  return carve_size((size_t)num_nodes * 2 * (H * F / (1 << proj_logw(F))) * sizeof(float)) + 256;
}

extern "C" int mvml_gat_proj_fwd(int64_t num_nodes, const float* X, int64_t ldx, int64_t K,
                                 const float* Wcat, int64_t ldw, const float* attn_lr, int H,
                                 int F, int mean_residual, int algo, float* Y, int64_t ldy,
                                 float* elr, const uint32_t* amax_x, const uint32_t* amax_w,
                                 const uint16_t* w_planes, int64_t w_plane, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  clear_error();
  MVML_REQUIRE(H == 1 || H == 2 || H == 4 || H == 8, "gat_proj_fwd: num_heads must be 1, 2, 4 or 8 (got %d)", H);
  MVML_REQUIRE(F > 0 && F % 4 == 0, "gat_proj_fwd: out_feats must be a positive multiple of 4 (got %d)", F);
  MVML_REQUIRE(num_nodes >= 0 && K > 0 && ldx >= K && ldw >= K, "gat_proj_fwd: bad shape");
  const int C = mvml_gat_proj_cols_res(H, F, mean_residual);  // (0 / 1, or MVML_RES_NONE)
  MVML_REQUIRE(ldy >= C, "gat_proj_fwd: ldy < %d", C);
  if (num_nodes == 0) return MVML_OK;
  if (!workspace || workspace_bytes < mvml_gat_proj_fwd_workspace_size(num_nodes, H, F)) {
    set_error("gat_proj_fwd: workspace of mvml_gat_proj_fwd_workspace_size bytes required");
    return MVML_ERR_WORKSPACE;
  }
  MVML_REQUIRE(attn_lr != nullptr && elr != nullptr, "gat_proj_fwd: attn_lr and elr are required");
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  MVML_REQUIRE(algo == MVML_GEMM_F32 || algo == MVML_GEMM_F32X3 || algo == MVML_GEMM_BF16 ||
                   algo == MVML_GEMM_F16X2,
               "gat_proj_fwd: bad algo %d", algo);
  uint32_t* amax_ws = reinterpret_cast<uint32_t*>(
      static_cast<uint8_t*>(workspace) +
      carve_size((size_t)num_nodes * 2 * (H * F / (1 << proj_logw(F))) * sizeof(float)));
  int rc = gemm_proj_epi(algo, num_nodes, C, K, X, ldx, Wcat, ldw, Y, ldy,
                         attn_lr, H * F, proj_logw(F), part, amax_ws, amax_x, amax_w, w_planes, st);
  if (rc) return rc;
  const int W = 1 << proj_logw(F);
  const unsigned blocks = (unsigned)ceil_div(num_nodes * 2 * H, 256);
  switch_const<1, 2, 4, 8>(H, [&](auto h) {  // (H: checked above)
    gat_logits_finalize_kernel<decltype(h)::value><<<blocks, 256, 0, st>>>(num_nodes, F, W, part, elr);
    return MVML_OK;
  });
  return check_launch("gat_logits_finalize_kernel");
}

extern "C" size_t mvml_gat_attn_grad_workspace_size(int64_t num_nodes, int H, int F) {
  return carve_size((size_t)attn_grad_splits(num_nodes, H * F) * 2 * H * F * sizeof(float));
}

extern "C" int mvml_gat_attn_grad(int64_t num_nodes, int H, int F, const float* Y, int64_t ldy,
                                  const float* gelr, int64_t ldgl, float* g_attn_l, float* g_attn_r,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  MVML_REQUIRE(H > 0 && F > 0 && num_nodes >= 0 && ldy >= (int64_t)H * F && ldgl >= 2 * H,
               "gat_attn_grad: bad shape");
  if (!workspace || workspace_bytes < mvml_gat_attn_grad_workspace_size(num_nodes, H, F)) {
    set_error("gat_attn_grad: workspace too small");
    return MVML_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int HF = H * F;
  const int S = attn_grad_splits(num_nodes, HF);
  const int64_t rows_per = ceil_div(num_nodes > 0 ? num_nodes : 1, S);
  float* part = static_cast<float*>(workspace);
  dim3 g1((unsigned)ceil_div(HF, 256), (unsigned)S);
  attn_grad_partial_kernel<<<g1, 256, 0, st>>>(num_nodes, H, F, Y, ldy, gelr, ldgl, rows_per, part);
  attn_grad_final_kernel<<<(unsigned)ceil_div(2 * HF, 256), 256, 0, st>>>(HF, S, part, g_attn_l, g_attn_r);
  return check_launch("attn_grad");
}

extern "C" int mvml_gat_fold_weights_res(const float* fc_w, const float* res_fc_w, const float* attn_lr,
                                         int H, int F, int Fin, int ldw, int res, float* Wcat,
                                         void* stream) {
  clear_error();
  MVML_REQUIRE(H > 0 && F > 0 && Fin > 0 && ldw >= Fin, "gat_fold_weights: bad shape");
  MVML_REQUIRE(res == MVML_RES_PROJ || res == MVML_RES_MEAN || res == MVML_RES_NONE,
               "gat_fold_weights: bad residual kind %d", res);
  MVML_REQUIRE(res == MVML_RES_NONE || res_fc_w != nullptr, "gat_fold_weights: res_fc_w is required");
  hipStream_t st = as_stream(stream);
  const int64_t total = (int64_t)(mvml_gat_proj_cols_res(H, F, res) + (attn_lr ? 2 * H : 0)) * ldw;
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(total, 256), 8192);
  fold_weights_kernel<<<blocks, 256, 0, st>>>(fc_w, res_fc_w, attn_lr, H, F, Fin, ldw, res, Wcat);
  return check_launch("fold_weights_kernel");
}

// (the entries without _res: the same checks, so a NULL res_fc_w / g_res_fc_w is refused there too)
extern "C" int mvml_gat_fold_weights(const float* fc_w, const float* res_fc_w, const float* attn_lr,
                                     int H, int F, int Fin, int ldw, int mean_residual, float* Wcat,
                                     void* stream) {
  return mvml_gat_fold_weights_res(fc_w, res_fc_w, attn_lr, H, F, Fin, ldw,
                                   mean_residual ? MVML_RES_MEAN : MVML_RES_PROJ, Wcat, stream);
}

extern "C" int mvml_gat_unfold_grads_res(const float* gWcat, const float* attn_lr, int H, int F,
                                         int Fin, int ldg, int res, float* g_fc_w, float* g_res_fc_w,
                                         void* stream) {
  clear_error();
  MVML_REQUIRE(H > 0 && F > 0 && Fin > 0 && ldg >= Fin, "gat_unfold_grads: bad shape");
  MVML_REQUIRE(res == MVML_RES_PROJ || res == MVML_RES_MEAN || res == MVML_RES_NONE,
               "gat_unfold_grads: bad residual kind %d", res);
  MVML_REQUIRE(res == MVML_RES_NONE || g_res_fc_w != nullptr, "gat_unfold_grads: g_res_fc_w is required");
  hipStream_t st = as_stream(stream);
  const int64_t total = (int64_t)H * F * Fin;
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(total, 256), 8192);
  unfold_w_kernel<<<blocks, 256, 0, st>>>(gWcat, attn_lr, H, F, Fin, ldg, res, g_fc_w, g_res_fc_w);
  return check_launch("unfold_w_kernel");
}

extern "C" int mvml_gat_unfold_grads(const float* gWcat, const float* attn_lr, int H, int F,
                                     int Fin, int ldg, int mean_residual, float* g_fc_w,
                                     float* g_res_fc_w, void* stream) {
  return mvml_gat_unfold_grads_res(gWcat, attn_lr, H, F, Fin, ldg,
                                   mean_residual ? MVML_RES_MEAN : MVML_RES_PROJ, g_fc_w, g_res_fc_w, stream);
}
