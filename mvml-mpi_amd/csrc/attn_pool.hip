// AttentiveFPReadout's softmax-weighted sum (dgllife 0.3.0 readout/attentivefp_readout.py
// GlobalPool; restated, parity with dgllife unpinned), conditioned on a per-graph state through u:
//
//   z_v = leaky(w_node . X[v] + u[b], slope)    a = softmax of z over the atoms of graph b
//   r[b] = sum_v a_v X[v]                       (project_nodes is applied to r at graph level)
//
// One wave per graph, lanes on the float4 columns c = lane + 64 j (D <= 1024: up to four slots),
// atoms in order with an online softmax: an atom row is read ONCE into registers, the logit's dot
// and the weighted sum both come from them.  Why a wave and not a workgroup per graph: molecules
// have 1 to ~400 atoms (a 400-atom graph is 400 iterations of one wave, microseconds), a batch has
// thousands of graphs, so waves alone fill the machine; a workgroup per graph would idle three
// waves on every small molecule and need an LDS merge of the partial softmaxes, whose order would
// depend on the split.  The raw logit of atom i is parked in attn_out by lane i % 64, which alone
// reads it back for the normalisation (no fence).
//
// Backward, no atomics: wave p walks the graphs of range p (mvml_attn_pool_partial_rows(B) ranges);
// per atom, again one read of the row: the recomputed w_node . x for the LeakyReLU side and c_v =
// g_r . (x_v - r[b]), recentred by its attention-weighted mean over the stored weights so that a
// graph's dz sum to 0 (dz_v = a_v leaky' (c_v - cbar)); c_v and a_v leaky' are parked per atom and a
// second pass over those scalars alone writes gX[v] (+)= a_v g_r[b] + dz_v w_node and g_u[b] =
// sum_v dz_v; the range's sum of dz x stays in registers (partial g_wn, mvml_colsum_f32).
#include "gat_agg_common.h"

namespace mvml {
namespace {

__device__ __forceinline__ float4 fma4_rn(float a, float4 x, float4 c) {
  return make_float4(__fmaf_rn(a, x.x, c.x), __fmaf_rn(a, x.y, c.y), __fmaf_rn(a, x.z, c.z),
                     __fmaf_rn(a, x.w, c.w));
}
__device__ __forceinline__ float4 scale4(float a, float4 x) {
  return make_float4(__fmul_rn(a, x.x), __fmul_rn(a, x.y), __fmul_rn(a, x.z), __fmul_rn(a, x.w));
}
__device__ __forceinline__ float4 add4_rn(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float wave_sum_rn(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

template <int NJ>
__global__ void __launch_bounds__(256)
attn_pool_fwd_kernel(int64_t B, int D, const int64_t* __restrict__ offs, const float* __restrict__ X, int64_t ldx,
                     const float* __restrict__ wn, const float* __restrict__ u, float slope, float* __restrict__ r_out,
                     int64_t ldr, float* __restrict__ attn) {
  const int lane = threadIdx.x & 63;
  const int64_t b = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= B) return;
  const int q = D / 4;
  bool ok[NJ];
  float4 w[NJ], acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    ok[j] = lane + 64 * j < q;
    w[j] = ok[j] ? ld4(wn + 4 * (lane + 64 * j)) : f4(0.f);
    acc[j] = f4(0.f);
  }
  const int64_t v0 = offs[b], v1 = offs[b + 1];
  const float ub = u[b];
  float m = -INFINITY, den = 0.f;
  for (int64_t v = v0; v < v1; ++v) {
    float4 x[NJ];
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      x[j] = ok[j] ? ld4nt(X + v * ldx + 4 * (lane + 64 * j)) : f4(0.f);
      part = __fadd_rn(part, dot4(w[j], x[j]));
    }
    const float z = leaky(__fadd_rn(wave_sum_rn(part), ub), slope);
    const float mn = fmaxf(m, z);
    const float sc = expf(m - mn), p = expf(z - mn);
    den = __fmaf_rn(den, sc, p);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = fma4_rn(p, x[j], scale4(sc, acc[j]));
    m = mn;
    if (lane == (int)((v - v0) & 63)) attn[v] = z;  // parked; this lane alone reads it back below
  }
  const float inv = v1 > v0 ? 1.f / den : 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (ok[j]) st4(r_out + b * ldr + 4 * (lane + 64 * j), scale4(inv, acc[j]));
  for (int64_t v = v0 + lane; v < v1; v += 64) attn[v] = __fmul_rn(expf(attn[v] - m), inv);
}

template <int NJ>
__global__ void __launch_bounds__(256)
attn_pool_bwd_kernel(int64_t B, int64_t Pn, int D, const int64_t* __restrict__ offs, const float* __restrict__ X,
                     int64_t ldx, const float* __restrict__ wn, const float* __restrict__ u, float slope,
                     const float* __restrict__ R, int64_t ldr, const float* __restrict__ attn,
                     const float* __restrict__ GR, int64_t ldgr, int accumulate, float* __restrict__ gX, int64_t ldgx,
                     float* __restrict__ g_u, float* __restrict__ cws, float* __restrict__ bws,
                     float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= Pn) return;
  const int q = D / 4;
  const int64_t per = ceil_div(B, Pn);
  const int64_t b0 = min(p * per, B), b1 = min(b0 + per, B);
  bool ok[NJ];
  float4 w[NJ], aw[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    ok[j] = lane + 64 * j < q;
    w[j] = ok[j] ? ld4(wn + 4 * (lane + 64 * j)) : f4(0.f);
    aw[j] = f4(0.f);
  }
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t v0 = offs[b], v1 = offs[b + 1];
    const float ub = u[b];
    // c_v = g_r . (x_v - r[b]) (the difference first), recentred by cbar = sum a c / sum a over the
    // stored weights, so the graph's d z sum to 0 as a softmax's do; b_v = a_v leaky'(pre_v),
    // d z_v = b_v (c_v - cbar), and the graph's sum of d z_v x_v is rw - cbar rv.
    float4 gr[NJ], rb[NJ], rw[NJ], rv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      gr[j] = ok[j] ? ld4(GR + b * ldgr + 4 * (lane + 64 * j)) : f4(0.f);
      rb[j] = ok[j] ? ld4(R + b * ldr + 4 * (lane + 64 * j)) : f4(0.f);
      rw[j] = rv[j] = f4(0.f);
    }
    float sa = 0.f, sc = 0.f;
    for (int64_t v = v0; v < v1; ++v) {
      float4 x[NJ];
      float d1 = 0.f, d2 = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        x[j] = ok[j] ? ld4nt(X + v * ldx + 4 * (lane + 64 * j)) : f4(0.f);
        d1 = __fadd_rn(d1, dot4(w[j], x[j]));
        d2 = __fadd_rn(d2, dot4(gr[j], make_float4(__fsub_rn(x[j].x, rb[j].x), __fsub_rn(x[j].y, rb[j].y),
                                                   __fsub_rn(x[j].z, rb[j].z), __fsub_rn(x[j].w, rb[j].w))));
      }
      d1 = wave_sum_rn(d1);
      d2 = wave_sum_rn(d2);
      const float a = attn[v];
      const float bv = __fadd_rn(d1, ub) > 0.f ? a : __fmul_rn(a, slope);
      sa = __fadd_rn(sa, a);
      sc = __fmaf_rn(a, d2, sc);
      if (lane == (int)((v - v0) & 63)) {  // parked; this lane alone reads them back below
        cws[v] = d2;
        bws[v] = bv;
      }
      const float bc = __fmul_rn(bv, d2);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        rw[j] = fma4_rn(bc, x[j], rw[j]);
        rv[j] = fma4_rn(bv, x[j], rv[j]);
      }
    }
    const float cbar = v1 > v0 ? sc / sa : 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) aw[j] = add4_rn(aw[j], fma4_rn(-cbar, rv[j], rw[j]));
    float gu = 0.f;
    for (int64_t base = v0; base < v1; base += 64) {  // no atom row is read again: a, d z, g_r and w_node only
      const int cnt = (int)min((int64_t)64, v1 - base);
      float dz_l = 0.f, a_l = 0.f;
      if (lane < cnt) {
        dz_l = __fmul_rn(bws[base + lane], __fsub_rn(cws[base + lane], cbar));
        a_l = attn[base + lane];
      }
      for (int i = 0; i < cnt; ++i) {
        const float dz = rl(dz_l, i), a = rl(a_l, i);
        gu = __fadd_rn(gu, dz);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (!ok[j]) continue;
          float* gx = gX + (base + i) * ldgx + 4 * (lane + 64 * j);
          float4 o = fma4_rn(a, gr[j], scale4(dz, w[j]));
          if (accumulate) o = add4_rn(ld4(gx), o);
          st4(gx, o);
        }
      }
    }
    if (lane == 0) g_u[b] = gu;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (ok[j]) st4(part + p * D + 4 * (lane + 64 * j), aw[j]);
}

inline int check_pool(const char* who, int64_t B, int64_t N, int D) {
  MVML_REQUIRE(B >= 0 && B < (int64_t(1) << 31) && N >= 0 && N < (int64_t(1) << 31), "%s: bad B %lld or N %lld", who,
               (long long)B, (long long)N);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024, "%s: D must be a positive multiple of 4 <= 1024 (got %d)", who, D);
  return MVML_OK;
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_attn_pool_fwd(int64_t B, int64_t N, int D, const int64_t* node_offsets, const float* X, int64_t ldx,
                                  const float* w_node, const float* u, float slope, float* r_out, int64_t ldr,
                                  float* attn_out, void* stream) {
  clear_error();
  if (int rc = check_pool("attn_pool_fwd", B, N, D)) return rc;
  if (B == 0) return MVML_OK;
  MVML_REQUIRE(node_offsets != nullptr && w_node != nullptr && aligned16(w_node) && u != nullptr && attn_out != nullptr,
               "attn_pool_fwd: node_offsets, 16-byte aligned w_node, u and attn_out are required");
  MVML_REQUIRE((N == 0 || row_ok(X, ldx, D)) && row_ok(r_out, ldr, D),
               "attn_pool_fwd: X and r_out must be 16-byte aligned with pitches >= D that are multiples of 4");
  const hipStream_t st = as_stream(stream);
  switch_const<1, 2, 3, 4>((int)ceil_div(D / 4, 64), [&](auto s) {
    attn_pool_fwd_kernel<decltype(s)::value><<<(unsigned)ceil_div(B, 4), 256, 0, st>>>(
        B, D, node_offsets, X, ldx, w_node, u, slope, r_out, ldr, attn_out);
    return MVML_OK;
  });
  return check_launch("attn_pool_fwd_kernel");
}

extern "C" int64_t mvml_attn_pool_partial_rows(int64_t B) {
  return std::min<int64_t>(std::max<int64_t>(B, 1), 4096);
}

extern "C" size_t mvml_attn_pool_bwd_workspace_size(int64_t B, int64_t N, int D) {
  if (B < 0 || N < 0 || D <= 0) return 0;
  const int64_t Pn = mvml_attn_pool_partial_rows(B);
  return carve_size((size_t)Pn * D * 4) + carve_size(mvml_colsum_workspace_size(Pn, D)) +
         2 * carve_size((size_t)std::max<int64_t>(N, 1) * 4) + 256;
}

extern "C" int mvml_attn_pool_bwd(int64_t B, int64_t N, int D, const int64_t* node_offsets, const float* X, int64_t ldx,
                                  const float* w_node, const float* u, float slope, const float* r_out, int64_t ldr,
                                  const float* attn, const float* g_r, int64_t ldgr, int accumulate, float* gX,
                                  int64_t ldgx, float* g_u, float* g_wn, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  clear_error();
  if (int rc = check_pool("attn_pool_bwd", B, N, D)) return rc;
  MVML_REQUIRE(g_wn != nullptr && aligned16(g_wn), "attn_pool_bwd: g_wn is required, 16-byte aligned");
  if (B == 0) return mvml_fill_zero(g_wn, 1, (int64_t)D * 4, (int64_t)D * 4, stream);
  MVML_REQUIRE(node_offsets != nullptr && w_node != nullptr && aligned16(w_node) && u != nullptr && attn != nullptr &&
                   g_u != nullptr,
               "attn_pool_bwd: node_offsets, 16-byte aligned w_node, u, attn and g_u are required");
  MVML_REQUIRE((N == 0 || (row_ok(X, ldx, D) && row_ok(gX, ldgx, D))) && row_ok(r_out, ldr, D) && row_ok(g_r, ldgr, D),
               "attn_pool_bwd: X, gX, r_out and g_r must be 16-byte aligned with pitches >= D that are multiples of 4");
  const size_t need = mvml_attn_pool_bwd_workspace_size(B, N, D);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("attn_pool_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  const int64_t Pn = mvml_attn_pool_partial_rows(B);
  Carver cv(workspace, workspace_bytes);
  float* part = cv.take<float>((size_t)Pn * D);
  const size_t cbytes = mvml_colsum_workspace_size(Pn, D);
  void* cws = cv.take<char>(cbytes);
  float* cpark = cv.take<float>((size_t)std::max<int64_t>(N, 1));
  float* bpark = cv.take<float>((size_t)std::max<int64_t>(N, 1));
  const hipStream_t st = as_stream(stream);
  switch_const<1, 2, 3, 4>((int)ceil_div(D / 4, 64), [&](auto s) {
    attn_pool_bwd_kernel<decltype(s)::value><<<(unsigned)ceil_div(Pn, 4), 256, 0, st>>>(
        B, Pn, D, node_offsets, X, ldx, w_node, u, slope, r_out, ldr, attn, g_r, ldgr, accumulate, gX, ldgx, g_u, cpark,
        bpark, part);
    return MVML_OK;
  });
  if (int rc = check_launch("attn_pool_bwd_kernel")) return rc;
  return mvml_colsum_f32(Pn, D, part, D, 1.f, 0.f, g_wn, cws, cbytes, stream);
}
