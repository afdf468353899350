// AttentiveFP's context layer (dgllife 0.3.0 gnn/attentivefp.py GetContext; restated, parity with
// dgllife unpinned): an edge softmax whose logits AND messages are functions of the bond row and
// the source atom row, with nothing of shape [E, G] in memory, forward or backward.
//
//   he_s = leaky(P[u] + b1 + sum_k e_s[k] W1eT[k])       P = x W1n^T (node-level GEMM), e_s the bond row
//   l_s  = leaky(t[v] + w2e . he_s)                      t = w2n . hv_new + b2 (per atom)
//   s[v] = sum_s softmax_v(l)_s he_s                     then c = We s + be [deg > 0] at node level
//
// Forward: a group of LW lanes owns a destination atom, lane s of it the float4 columns s + LW j
// (LW = 64, up to four slots, G <= 1024; G <= 64: LW = 16, four atoms per wave).  One pass over the
// in-slots with an online softmax (running max, denominator, rescaled accumulator); the logit's
// dot is a butterfly over the group's lanes per edge.  W1eT ([De][G]) is staged in LDS once per
// workgroup where it fits kAfpLdsBytes, each group then walking kAfpRows atoms; otherwise every
// lane reads its float4 of a W1eT row from L2 (coalesced over the lanes).  The raw logit of slot j
// is parked in attn_out by lane j % LW, which alone re-reads it for the final normalisation, so no
// fence is needed.  he_s is formed by q_of() in every kernel of this file: the same fmas in the
// same order, so the backward's LeakyReLU sides are the forward's.
//
// Backward, no float atomics: stage 1 by destination atom (one wave each, a contiguous atom range
// per wave) recomputes he_s, takes the softmax backward through g_s . (he_s - s[v]), recentred by
// its own attention-weighted mean so that a row's d l sum to 0 with the STORED weights, writes
// d_pre per slot and g_t per atom and keeps the range's sum of d_pre he_s in registers (partial
// g_w2e).  Stage 2 by source atom over the out-CSR is separable by column, so its grid is (atom
// range) x (256-column chunk): a lane holds ONE float4 column slot and the 4 ceil(De / 4)
// accumulators of g_W1eT for it in registers (De <= 32: 128 registers at most), its chunk of W1eT
// in LDS (De KiB).  Both stages' partials go through mvml_colsum_f32.
#include "gat_agg_common.h"

namespace mvml {
namespace {

constexpr int kAfpMaxDe = 32;
constexpr int kAfpLdsBytes = 48 * 1024;  // staged W1eT: three workgroups per CU keep theirs
constexpr int kAfpRows = 8;              // atoms a lane group walks per staged copy
constexpr int kAfpSubG = 64;             // G <= 64: 16 lanes per atom, four atoms per wave
constexpr float kAfpSlope = 0.01f;       // torch's LeakyReLU default, AttentiveFP's everywhere

__device__ __forceinline__ float4 add4_rn(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float4 fma4_rn(float a, float4 x, float4 c) {
  return make_float4(__fmaf_rn(a, x.x, c.x), __fmaf_rn(a, x.y, c.y), __fmaf_rn(a, x.z, c.z),
                     __fmaf_rn(a, x.w, c.w));
}
__device__ __forceinline__ float4 leaky4(float4 q) {
  return make_float4(leaky(q.x, kAfpSlope), leaky(q.y, kAfpSlope), leaky(q.z, kAfpSlope), leaky(q.w, kAfpSlope));
}
__device__ __forceinline__ float4 scale4(float a, float4 x) {
  return make_float4(__fmul_rn(a, x.x), __fmul_rn(a, x.y), __fmul_rn(a, x.z), __fmul_rn(a, x.w));
}
template <int LW>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = LW / 2; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}
template <int LW>
__device__ __forceinline__ int groups_max(int x) {  // over a wave's groups, x uniform in each
  if (LW < 64) {
    x = max(x, __shfl_xor(x, 16, 64));
    x = max(x, __shfl_xor(x, 32, 64));
  }
  return x;
}

// The pre-activation of he for one float4 column slot: (p + b1) + e[0] W[0] + e[1] W[1] + ...,
// W[k] = w[k * stride] (LDS or global), brow the slot's padded bond row.
__device__ __forceinline__ float4 q_of(float4 p, float4 b1, const float* __restrict__ brow, int De,
                                       const float4* w, int stride) {
  float4 q = add4_rn(p, b1);
  for (int k0 = 0; k0 < De; k0 += 4) {
    const float4 e = ld4(brow + k0);
    q = fma4_rn(e.x, w[(k0 + 0) * stride], q);
    if (k0 + 1 < De) q = fma4_rn(e.y, w[(k0 + 1) * stride], q);
    if (k0 + 2 < De) q = fma4_rn(e.z, w[(k0 + 2) * stride], q);
    if (k0 + 3 < De) q = fma4_rn(e.w, w[(k0 + 3) * stride], q);
  }
  return q;
}

// One thread per float4 of rows.
__global__ void __launch_bounds__(256)
afp_edge_rows_kernel(int64_t E, int De, int Dp, const int32_t* __restrict__ in_eid, const float* __restrict__ e,
                     int64_t lde, float* __restrict__ rows) {
  const int q = Dp / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E * q) return;
  const int64_t s = i / q;
  const int c = 4 * (int)(i - s * q);
  int eid = in_eid[s];
  if (eid < 0 || eid >= E) eid = 0;  // not an index of mvml_build_csr: read as edge 0
  const float* src = e + (int64_t)eid * lde;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = c + k < De ? src[c + k] : 0.f;
  st4(rows + s * Dp + c, make_float4(v[0], v[1], v[2], v[3]));
}

struct AfpArgs {
  int64_t N;
  const int32_t *rowptr, *nbr;
  const float* P;
  int64_t ldp;
  int G;
  const float* brows;
  int De, Dp;
  const float *W1eT, *b1, *w2e, *t;
};

template <int NJ, int LW, bool LDS>
__global__ void __launch_bounds__(256)
afp_context_fwd_kernel(AfpArgs a, float* __restrict__ s_out, int64_t lds_o, float* __restrict__ attn) {
  extern __shared__ float4 s_w[];  // LDS: [De][G / 4]
  const int q = a.G / 4;
  if (LDS) {
    for (int i = threadIdx.x; i < a.De * q; i += 256) s_w[i] = ld4(a.W1eT + 4 * (int64_t)i);
    __syncthreads();
  }
  constexpr int GPB = 256 / LW;
  constexpr int RPG = LDS ? kAfpRows : 1;
  const int lane = threadIdx.x & 63, sl = lane & (LW - 1), g0 = lane & ~(LW - 1);
  const int64_t r0 = (xcd_block(blockIdx.x, gridDim.x) * GPB + threadIdx.x / LW) * RPG;
  bool ok[NJ];
  float4 b1r[NJ], w2r[NJ];
  const float4* wcol[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int ci = sl + LW * j;
    ok[j] = ci < q;
    b1r[j] = ok[j] ? ld4(a.b1 + 4 * ci) : f4(0.f);
    w2r[j] = ok[j] ? ld4(a.w2e + 4 * ci) : f4(0.f);
    wcol[j] = (LDS ? s_w : reinterpret_cast<const float4*>(a.W1eT)) + (ok[j] ? ci : 0);
  }
  for (int i = 0; i < RPG; ++i) {
    const int64_t v = r0 + i;
    const bool row = v < a.N;
    if (__ballot(row) == 0) break;  // (uniform; no barrier below)
    int eb = 0, deg = 0;
    float tv = 0.f;
    if (row) {
      eb = a.rowptr[v];
      deg = a.rowptr[v + 1] - eb;
      tv = a.t[v];
    }
    const int mdeg = groups_max<LW>(deg);
    float m = -INFINITY, den = 0.f;
    float4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f4(0.f);
    int id_l = 0;
    for (int e = 0; e < mdeg; ++e) {
      const int el = e & (LW - 1);
      if (el == 0) id_l = e + sl < deg ? a.nbr[eb + e + sl] : 0;
      const int u = __shfl(id_l, g0 + el, 64);
      const bool act = e < deg;
      float4 he[NJ];
      float part = 0.f;
      const float* brow = a.brows + (int64_t)(eb + (act ? e : 0)) * a.Dp;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        he[j] = f4(0.f);
        if (act && ok[j]) {
          const float4 p = ld4(a.P + (int64_t)u * a.ldp + 4 * (sl + LW * j));
          he[j] = leaky4(q_of(p, b1r[j], brow, a.De, wcol[j], q));
          part = __fadd_rn(part, dot4(w2r[j], he[j]));
        }
      }
      const float dot = group_sum<LW>(part);
      if (act) {
        const float l = leaky(__fadd_rn(tv, dot), kAfpSlope);
        const float mn = fmaxf(m, l);
        const float sc = expf(m - mn), p = expf(l - mn);
        den = __fmaf_rn(den, sc, p);
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = fma4_rn(p, he[j], scale4(sc, acc[j]));
        m = mn;
        if (sl == el) attn[eb + e] = l;  // parked; this lane alone reads it back below
      }
    }
    if (row) {
      const float inv = deg > 0 ? 1.f / den : 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (ok[j]) st4nt(s_out + v * lds_o + 4 * (sl + LW * j), scale4(inv, acc[j]));
      for (int e = sl; e < deg; e += LW) attn[eb + e] = __fmul_rn(expf(attn[eb + e] - m), inv);
    }
  }
}

// Stage 1 of the backward: wave p walks the destination atoms of range p.
template <int NJ, bool LDS>
__global__ void __launch_bounds__(256)
afp_context_bwd_dst_kernel(AfpArgs a, int64_t Pn, const float* __restrict__ S, int64_t lds_o,
                           const float* __restrict__ attn, const float* __restrict__ GS, int64_t ldgs,
                           float* __restrict__ dpre, float* __restrict__ bws, float* __restrict__ g_t,
                           float* __restrict__ part) {
  extern __shared__ float4 s_w[];
  const int q = a.G / 4;
  if (LDS) {
    for (int i = threadIdx.x; i < a.De * q; i += 256) s_w[i] = ld4(a.W1eT + 4 * (int64_t)i);
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= Pn) return;
  const int64_t per = ceil_div(a.N, Pn);
  const int64_t a0 = min(p * per, a.N), a1 = min(a0 + per, a.N);
  bool ok[NJ];
  float4 b1r[NJ], w2r[NJ], aw[NJ];
  const float4* wcol[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int ci = lane + 64 * j;
    ok[j] = ci < q;
    b1r[j] = ok[j] ? ld4(a.b1 + 4 * ci) : f4(0.f);
    w2r[j] = ok[j] ? ld4(a.w2e + 4 * ci) : f4(0.f);
    wcol[j] = (LDS ? s_w : reinterpret_cast<const float4*>(a.W1eT)) + (ok[j] ? ci : 0);
    aw[j] = f4(0.f);
  }
  for (int64_t v = a0; v < a1; ++v) {
    const int eb = a.rowptr[v], deg = a.rowptr[v + 1] - eb;
    const float tv = a.t[v];
    float4 gs[NJ], sv[NJ];  // d a = g_s . (he - s[v]): the difference first, so a dominant edge's cancels exactly
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      gs[j] = ok[j] ? ld4(GS + v * ldgs + 4 * (lane + 64 * j)) : f4(0.f);
      sv[j] = ok[j] ? ld4(S + v * lds_o + 4 * (lane + 64 * j)) : f4(0.f);
    }
    // c_e = g_s . (he_e - s[v]) is recentred by cbar = sum_e a_e c_e / sum_e a_e (tiny: what the stored
    // a and s disagree by), so the d l_e = a_e (c_e - cbar) of a row sum to 0 as the softmax's do.  With
    // b_e = a_e leaky'(pre_e): d_pre_e = b_e (c_e - cbar), and the row's sum of d_pre_e he_e is
    // rw - cbar rv, rw = sum_e b_e c_e he_e, rv = sum_e b_e he_e.  The row's own sum first: its d_pre
    // cancel, the range's do not.
    float sa = 0.f, sc = 0.f;
    float4 rw[NJ], rv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) rw[j] = rv[j] = f4(0.f);
    for (int base = 0; base < deg; base += 64) {
      const int cnt = min(64, deg - base);
      const int id_l = lane < cnt ? a.nbr[eb + base + lane] : 0;
      for (int e = 0; e < cnt; ++e) {
        const int u = rl(id_l, e);
        const float* brow = a.brows + (int64_t)(eb + base + e) * a.Dp;
        float4 he[NJ];
        float d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          he[j] = f4(0.f);
          if (ok[j]) {
            const float4 pu = ld4(a.P + (int64_t)u * a.ldp + 4 * (lane + 64 * j));
            he[j] = leaky4(q_of(pu, b1r[j], brow, a.De, wcol[j], q));
            d1 = __fadd_rn(d1, dot4(w2r[j], he[j]));
            d2 = __fadd_rn(d2, dot4(gs[j], make_float4(__fsub_rn(he[j].x, sv[j].x), __fsub_rn(he[j].y, sv[j].y),
                                                       __fsub_rn(he[j].z, sv[j].z), __fsub_rn(he[j].w, sv[j].w))));
          }
        }
        d1 = group_sum<64>(d1);
        d2 = group_sum<64>(d2);
        const float at = attn[eb + base + e];
        const float b = __fadd_rn(tv, d1) > 0.f ? at : __fmul_rn(at, kAfpSlope);
        sa = __fadd_rn(sa, at);
        sc = __fmaf_rn(at, d2, sc);
        if (lane == e) {  // parked; this lane alone reads them back below
          dpre[eb + base + e] = d2;
          bws[eb + base + e] = b;
        }
        const float bc = __fmul_rn(b, d2);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          rw[j] = fma4_rn(bc, he[j], rw[j]);
          rv[j] = fma4_rn(b, he[j], rv[j]);
        }
      }
    }
    const float cbar = deg > 0 ? sc / sa : 0.f;
    float gt = 0.f;
    for (int e = lane; e < deg; e += 64) {
      const float dp = __fmul_rn(bws[eb + e], __fsub_rn(dpre[eb + e], cbar));
      dpre[eb + e] = dp;
      gt = __fadd_rn(gt, dp);
    }
    gt = group_sum<64>(gt);
#pragma unroll
    for (int j = 0; j < NJ; ++j) aw[j] = add4_rn(aw[j], fma4_rn(-cbar, rv[j], rw[j]));
    if (lane == 0) g_t[v] = gt;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (ok[j]) st4(part + p * a.G + 4 * (lane + 64 * j), aw[j]);
}

// Stage 2: wave (p, chunk) walks the source atoms of range p for the 256 columns of its chunk.
template <int D4>
__global__ void __launch_bounds__(256)
afp_context_bwd_src_kernel(AfpArgs a, int64_t Pn, const int32_t* __restrict__ out_rowptr,
                           const int32_t* __restrict__ out_dst, const int32_t* __restrict__ out_inslot,
                           const float* __restrict__ attn, const float* __restrict__ dpre,
                           const float* __restrict__ GS, int64_t ldgs, float* __restrict__ gP, int64_t ldgp,
                           float* __restrict__ part) {
  __shared__ float4 s_w[kAfpMaxDe * 64];  // [De][64]: this chunk's columns of W1eT
  const int lane = threadIdx.x & 63;
  const int q = a.G / 4;
  const int ci = blockIdx.y * 64 + lane;
  const bool ok = ci < q;
  for (int i = threadIdx.x; i < a.De * 64; i += 256) {
    const int k = i >> 6, c = blockIdx.y * 64 + (i & 63);
    s_w[i] = c < q ? ld4(a.W1eT + (int64_t)k * a.G + 4 * c) : f4(0.f);
  }
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= Pn) return;
  const int64_t per = ceil_div(a.N, Pn);
  const int64_t a0 = min(p * per, a.N), a1 = min(a0 + per, a.N);
  const float4 b1r = ok ? ld4(a.b1 + 4 * ci) : f4(0.f);
  const float4 w2r = ok ? ld4(a.w2e + 4 * ci) : f4(0.f);
  float4 accw[4 * D4], accb = f4(0.f);
#pragma unroll
  for (int k = 0; k < 4 * D4; ++k) accw[k] = f4(0.f);
  for (int64_t u = a0; u < a1; ++u) {
    const int ob = out_rowptr[u], od = out_rowptr[u + 1] - ob;
    const float4 pu = ok ? ld4(a.P + u * a.ldp + 4 * ci) : f4(0.f);
    float4 gp = f4(0.f);
    for (int base = 0; base < od; base += 64) {
      const int cnt = min(64, od - base);
      const int v_l = lane < cnt ? out_dst[ob + base + lane] : 0;
      const int s_l = lane < cnt ? out_inslot[ob + base + lane] : 0;
      for (int e = 0; e < cnt; ++e) {
        const int v = rl(v_l, e), s = rl(s_l, e);
        const float* brow = a.brows + (int64_t)s * a.Dp;
        const float at = attn[s], dp = dpre[s];
        const float4 g = ok ? ld4(GS + (int64_t)v * ldgs + 4 * ci) : f4(0.f);
        const float4 qv = q_of(pu, b1r, brow, a.De, s_w + lane, 64);
        float4 dq = fma4_rn(at, g, scale4(dp, w2r));
        dq.x = qv.x > 0.f ? dq.x : __fmul_rn(dq.x, kAfpSlope);
        dq.y = qv.y > 0.f ? dq.y : __fmul_rn(dq.y, kAfpSlope);
        dq.z = qv.z > 0.f ? dq.z : __fmul_rn(dq.z, kAfpSlope);
        dq.w = qv.w > 0.f ? dq.w : __fmul_rn(dq.w, kAfpSlope);
        gp = add4_rn(gp, dq);
        accb = add4_rn(accb, dq);
#pragma unroll
        for (int k4 = 0; k4 < D4; ++k4) {
          const float4 ev = ld4(brow + 4 * k4);  // (pad entries are 0: their rows stay 0)
          accw[4 * k4 + 0] = fma4_rn(ev.x, dq, accw[4 * k4 + 0]);
          accw[4 * k4 + 1] = fma4_rn(ev.y, dq, accw[4 * k4 + 1]);
          accw[4 * k4 + 2] = fma4_rn(ev.z, dq, accw[4 * k4 + 2]);
          accw[4 * k4 + 3] = fma4_rn(ev.w, dq, accw[4 * k4 + 3]);
        }
      }
    }
    if (ok) st4(gP + u * ldgp + 4 * ci, gp);
  }
  if (ok) {
    float* pr = part + p * (int64_t)(a.De + 1) * a.G + 4 * ci;
#pragma unroll
    for (int k = 0; k < 4 * D4; ++k)
      if (k < a.De) st4(pr + (int64_t)k * a.G, accw[k]);
    st4(pr + (int64_t)a.De * a.G, accb);
  }
}

// One thread per float4 of the [N][G] rows.
template <bool BWD>
__global__ void __launch_bounds__(256)
afp_bias_elu_kernel(int64_t N, int G, const int32_t* __restrict__ rowptr, const float* __restrict__ in, int64_t ldi,
                    const float* __restrict__ bias, const float* __restrict__ g, int64_t ldg,
                    float* __restrict__ out, int64_t ldo) {
  const int q = G / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * q) return;
  const int64_t v = i / q;
  const int c = 4 * (int)(i - v * q);
  const bool on = rowptr == nullptr || rowptr[v + 1] > rowptr[v];
  const float4 x = ld4(in + v * ldi + c);
  if (BWD) {  // in = the forward's output: elu' = 1 (out > 0) else out + 1
    const float4 gv = ld4(g + v * ldg + c);
    st4(out + v * ldo + c, on ? make_float4(gv.x * (x.x > 0.f ? 1.f : x.x + 1.f), gv.y * (x.y > 0.f ? 1.f : x.y + 1.f),
                                            gv.z * (x.z > 0.f ? 1.f : x.z + 1.f), gv.w * (x.w > 0.f ? 1.f : x.w + 1.f))
                              : f4(0.f));
  } else {
    const float4 b = (on && bias != nullptr) ? ld4(bias + c) : f4(0.f);
    st4(out + v * ldo + c, make_float4(elu(x.x + b.x), elu(x.y + b.y), elu(x.z + b.z), elu(x.w + b.w)));
  }
}

template <bool BWD>
__global__ void __launch_bounds__(256)
leaky_rows_kernel(int64_t rows, int cols, const float* __restrict__ x, int64_t ldx, const float* __restrict__ g,
                  int64_t ldg, float* __restrict__ y, int64_t ldy, float slope) {
  const int q = cols / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * q) return;
  const int64_t r = i / q;
  const int c = 4 * (int)(i - r * q);
  const float4 a = ld4(x + r * ldx + c);
  if (BWD) {  // x = the forward's output: its sign is the input's
    const float4 gv = ld4(g + r * ldg + c);
    st4(y + r * ldy + c, make_float4(a.x > 0.f ? gv.x : gv.x * slope, a.y > 0.f ? gv.y : gv.y * slope,
                                     a.z > 0.f ? gv.z : gv.z * slope, a.w > 0.f ? gv.w : gv.w * slope));
  } else {
    st4(y + r * ldy + c, make_float4(leaky(a.x, slope), leaky(a.y, slope), leaky(a.z, slope), leaky(a.w, slope)));
  }
}

inline int check_afp(const char* who, int64_t N, int G, int De) {
  MVML_REQUIRE(N >= 0 && N < (int64_t(1) << 31), "%s: bad num_nodes %lld", who, (long long)N);
  MVML_REQUIRE(G > 0 && G % 4 == 0 && G <= 1024, "%s: G must be a positive multiple of 4 <= 1024 (got %d)", who, G);
  MVML_REQUIRE(De >= 1 && De <= kAfpMaxDe, "%s: 1 <= De <= 32 bond features (got %d)", who, De);
  return MVML_OK;
}
inline bool afp_lds(int G, int De) { return (size_t)De * G * 4 <= (size_t)kAfpLdsBytes; }

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_afp_edge_rows(int64_t num_edges, int De, const int32_t* in_eid, const float* e, int64_t lde,
                                  float* rows, void* stream) {
  clear_error();
  MVML_REQUIRE(num_edges >= 0 && num_edges < (int64_t(1) << 31), "afp_edge_rows: bad num_edges %lld",
               (long long)num_edges);
  MVML_REQUIRE(De >= 1 && De <= kAfpMaxDe, "afp_edge_rows: 1 <= De <= 32 bond features (got %d)", De);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(in_eid != nullptr && e != nullptr && lde >= De && rows != nullptr && aligned16(rows),
               "afp_edge_rows: in_eid, e (pitch >= De) and 16-byte aligned rows are required");
  const int Dp = (De + 3) / 4 * 4;
  afp_edge_rows_kernel<<<(unsigned)ceil_div(num_edges * (Dp / 4), 256), 256, 0, as_stream(stream)>>>(
      num_edges, De, Dp, in_eid, e, lde, rows);
  return check_launch("afp_edge_rows_kernel");
}

extern "C" int mvml_afp_context_fwd(int64_t num_nodes, const int32_t* in_rowptr, const int32_t* in_src,
                                    const float* P, int64_t ldp, int G, const float* bond_rows, int De,
                                    const float* W1eT, const float* b1, const float* w2e, const float* t,
                                    float* s_out, int64_t lds, float* attn_out, void* stream) {
  clear_error();
  if (int rc = check_afp("afp_context_fwd", num_nodes, G, De)) return rc;
  MVML_REQUIRE(row_ok(P, ldp, G) && row_ok(s_out, lds, G),
               "afp_context_fwd: P and s_out must be 16-byte aligned with row strides >= G that are multiples of 4");
  MVML_REQUIRE(W1eT != nullptr && b1 != nullptr && w2e != nullptr && aligned16(W1eT) && aligned16(b1) && aligned16(w2e),
               "afp_context_fwd: W1eT, b1 and w2e are required, 16-byte aligned");
  if (num_nodes == 0) return MVML_OK;
  // in_src, attn_out and bond_rows are touched per in-edge only: a batch without any bond passes its
  // empty arrays (NULL from an empty tensor), as the GAT aggregation lets it
  MVML_REQUIRE(in_rowptr != nullptr && t != nullptr && aligned16(bond_rows),
               "afp_context_fwd: in_rowptr and t are required, bond_rows 16-byte aligned");
  const hipStream_t st = as_stream(stream);
  const AfpArgs a{num_nodes, in_rowptr, in_src, P, ldp, G, bond_rows, De, (De + 3) / 4 * 4, W1eT, b1, w2e, t};
  const bool lds_w = afp_lds(G, De);
  const size_t wb = lds_w ? (size_t)De * G * 4 : 0;
  const int rpg = lds_w ? kAfpRows : 1;
  if (G <= kAfpSubG) {
    const unsigned nb = (unsigned)ceil_div(num_nodes, 16 * rpg);
    if (lds_w) afp_context_fwd_kernel<1, 16, true><<<nb, 256, wb, st>>>(a, s_out, lds, attn_out);
    else afp_context_fwd_kernel<1, 16, false><<<nb, 256, 0, st>>>(a, s_out, lds, attn_out);
  } else switch_const<1, 2, 3, 4>((int)ceil_div(G / 4, 64), [&](auto s) {
    constexpr int NJ = decltype(s)::value;
    const unsigned nb = (unsigned)ceil_div(num_nodes, 4 * rpg);
    if (lds_w) afp_context_fwd_kernel<NJ, 64, true><<<nb, 256, wb, st>>>(a, s_out, lds, attn_out);
    else afp_context_fwd_kernel<NJ, 64, false><<<nb, 256, 0, st>>>(a, s_out, lds, attn_out);
    return MVML_OK;
  });
  return check_launch("afp_context_fwd_kernel");
}

extern "C" int64_t mvml_afp_partial_rows(int64_t num_nodes) {
  return std::min<int64_t>(std::max<int64_t>(ceil_div(num_nodes, 64), 1), 4096);
}

extern "C" size_t mvml_afp_context_bwd_workspace_size(int64_t num_nodes, int64_t num_edges, int G, int De) {
  if (num_nodes < 0 || num_edges < 0 || G <= 0 || De <= 0) return 0;
  const int64_t Pn = mvml_afp_partial_rows(num_nodes);
  const int64_t wide = (int64_t)(De + 1) * G;
  return 2 * carve_size((size_t)std::max<int64_t>(num_edges, 1) * 4) + carve_size((size_t)Pn * G * 4) +
         carve_size((size_t)Pn * wide * 4) + carve_size(mvml_colsum_workspace_size(Pn, wide)) + 256;
}

extern "C" int mvml_afp_context_bwd(int64_t num_nodes, int64_t num_edges, const int32_t* in_rowptr,
                                    const int32_t* in_src, const int32_t* out_rowptr, const int32_t* out_dst,
                                    const int32_t* out_inslot, const float* P, int64_t ldp, int G,
                                    const float* bond_rows, int De, const float* W1eT, const float* b1,
                                    const float* w2e, const float* t, const float* s_out, int64_t lds,
                                    const float* attn, const float* g_s, int64_t ldgs, float* gP, int64_t ldgp,
                                    float* g_t, float* g_w2e, float* g_w1e_b1, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  clear_error();
  if (int rc = check_afp("afp_context_bwd", num_nodes, G, De)) return rc;
  MVML_REQUIRE(num_edges >= 0 && num_edges < (int64_t(1) << 31), "afp_context_bwd: bad num_edges %lld",
               (long long)num_edges);
  MVML_REQUIRE(row_ok(P, ldp, G) && row_ok(s_out, lds, G) && row_ok(g_s, ldgs, G) && row_ok(gP, ldgp, G),
               "afp_context_bwd: P, s_out, g_s and gP must be 16-byte aligned with row strides >= G that are "
               "multiples of 4");
  MVML_REQUIRE(W1eT != nullptr && b1 != nullptr && w2e != nullptr && aligned16(W1eT) && aligned16(b1) && aligned16(w2e),
               "afp_context_bwd: W1eT, b1 and w2e are required, 16-byte aligned");
  MVML_REQUIRE(g_w2e != nullptr && g_w1e_b1 != nullptr && aligned16(g_w2e) && aligned16(g_w1e_b1),
               "afp_context_bwd: g_w2e and g_w1e_b1 are required, 16-byte aligned");
  const int64_t wide = (int64_t)(De + 1) * G;
  if (num_nodes == 0) {
    if (int rc = mvml_fill_zero(g_w2e, 1, (int64_t)G * 4, (int64_t)G * 4, stream)) return rc;
    return mvml_fill_zero(g_w1e_b1, 1, wide * 4, wide * 4, stream);
  }
  MVML_REQUIRE(in_rowptr != nullptr && out_rowptr != nullptr && t != nullptr && g_t != nullptr,
               "afp_context_bwd: both row pointer arrays, t and g_t are required");
  MVML_REQUIRE(num_edges == 0 || (in_src != nullptr && out_dst != nullptr && out_inslot != nullptr && attn != nullptr &&
                                  bond_rows != nullptr && aligned16(bond_rows)),
               "afp_context_bwd: with edges, in_src, out_dst, out_inslot, attn and 16-byte aligned bond_rows are required");
  const size_t need = mvml_afp_context_bwd_workspace_size(num_nodes, num_edges, G, De);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("afp_context_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  const int64_t Pn = mvml_afp_partial_rows(num_nodes);
  Carver cv(workspace, workspace_bytes);
  float* dpre = cv.take<float>((size_t)std::max<int64_t>(num_edges, 1));
  float* bws = cv.take<float>((size_t)std::max<int64_t>(num_edges, 1));
  float* part1 = cv.take<float>((size_t)Pn * G);
  float* part2 = cv.take<float>((size_t)Pn * wide);
  const size_t cbytes = mvml_colsum_workspace_size(Pn, wide);
  void* cws = cv.take<char>(cbytes);
  const hipStream_t st = as_stream(stream);
  const AfpArgs a{num_nodes, in_rowptr, in_src, P, ldp, G, bond_rows, De, (De + 3) / 4 * 4, W1eT, b1, w2e, t};
  const bool lds_w = afp_lds(G, De);
  const size_t wb = lds_w ? (size_t)De * G * 4 : 0;
  const unsigned nb = (unsigned)ceil_div(Pn, 4);
  switch_const<1, 2, 3, 4>((int)ceil_div(G / 4, 64), [&](auto s) {
    constexpr int NJ = decltype(s)::value;
    if (lds_w)
      afp_context_bwd_dst_kernel<NJ, true><<<nb, 256, wb, st>>>(a, Pn, s_out, lds, attn, g_s, ldgs, dpre, bws,
                                                                g_t, part1);
    else
      afp_context_bwd_dst_kernel<NJ, false><<<nb, 256, 0, st>>>(a, Pn, s_out, lds, attn, g_s, ldgs, dpre, bws,
                                                                g_t, part1);
    return MVML_OK;
  });
  if (int rc = check_launch("afp_context_bwd_dst_kernel")) return rc;
  const dim3 grid(nb, (unsigned)ceil_div(G, 256));
  switch_const<1, 2, 3, 4, 5, 6, 7, 8>((De + 3) / 4, [&](auto s) {
    afp_context_bwd_src_kernel<decltype(s)::value><<<grid, 256, 0, st>>>(a, Pn, out_rowptr, out_dst, out_inslot, attn,
                                                                        dpre, g_s, ldgs, gP, ldgp, part2);
    return MVML_OK;
  });
  if (int rc = check_launch("afp_context_bwd_src_kernel")) return rc;
  if (int rc = mvml_colsum_f32(Pn, G, part1, G, 1.f, 0.f, g_w2e, cws, cbytes, stream)) return rc;
  return mvml_colsum_f32(Pn, wide, part2, wide, 1.f, 0.f, g_w1e_b1, cws, cbytes, stream);
}

extern "C" int mvml_afp_bias_elu(int64_t num_nodes, int G, const int32_t* in_rowptr, float* X, int64_t ldx,
                                 const float* bias, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && G > 0 && G % 4 == 0, "afp_bias_elu: bad shape %lld x %d", (long long)num_nodes, G);
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(row_ok(X, ldx, G) && aligned16(bias), "afp_bias_elu: X (pitch >= G, multiple of 4) and bias 16-byte aligned");
  afp_bias_elu_kernel<false><<<(unsigned)ceil_div(num_nodes * (G / 4), 256), 256, 0, as_stream(stream)>>>(
      num_nodes, G, in_rowptr, X, ldx, bias, nullptr, 0, X, ldx);
  return check_launch("afp_bias_elu_kernel");
}

extern "C" int mvml_afp_bias_elu_bwd(int64_t num_nodes, int G, const int32_t* in_rowptr, const float* out, int64_t ldo,
                                     const float* g, int64_t ldg, float* gX, int64_t ldgx, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && G > 0 && G % 4 == 0, "afp_bias_elu_bwd: bad shape %lld x %d", (long long)num_nodes, G);
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(row_ok(out, ldo, G) && row_ok(g, ldg, G) && row_ok(gX, ldgx, G),
               "afp_bias_elu_bwd: out, g and gX must be 16-byte aligned with pitches >= G that are multiples of 4");
  afp_bias_elu_kernel<true><<<(unsigned)ceil_div(num_nodes * (G / 4), 256), 256, 0, as_stream(stream)>>>(
      num_nodes, G, in_rowptr, out, ldo, nullptr, g, ldg, gX, ldgx);
  return check_launch("afp_bias_elu_bwd_kernel");
}

extern "C" int mvml_leaky_f32(int64_t rows, int cols, const float* x, int64_t ldx, float* y, int64_t ldy, float slope,
                              void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && cols > 0 && cols % 4 == 0, "leaky_f32: bad shape %lld x %d", (long long)rows, cols);
  if (rows == 0) return MVML_OK;
  MVML_REQUIRE(row_ok(x, ldx, cols) && row_ok(y, ldy, cols),
               "leaky_f32: x and y must be 16-byte aligned with pitches >= cols that are multiples of 4");
  leaky_rows_kernel<false><<<(unsigned)ceil_div(rows * (cols / 4), 256), 256, 0, as_stream(stream)>>>(
      rows, cols, x, ldx, nullptr, 0, y, ldy, slope);
  return check_launch("leaky_rows_kernel");
}

extern "C" int mvml_leaky_bwd_f32(int64_t rows, int cols, const float* y, int64_t ldy, const float* g, int64_t ldg,
                                  float* gx, int64_t ldgx, float slope, void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && cols > 0 && cols % 4 == 0, "leaky_bwd_f32: bad shape %lld x %d", (long long)rows, cols);
  if (rows == 0) return MVML_OK;
  MVML_REQUIRE(row_ok(y, ldy, cols) && row_ok(g, ldg, cols) && row_ok(gx, ldgx, cols),
               "leaky_bwd_f32: y, g and gx must be 16-byte aligned with pitches >= cols that are multiples of 4");
  leaky_rows_kernel<true><<<(unsigned)ceil_div(rows * (cols / 4), 256), 256, 0, as_stream(stream)>>>(
      rows, cols, y, ldy, g, ldg, gx, ldgx, slope);
  return check_launch("leaky_rows_kernel");
}
