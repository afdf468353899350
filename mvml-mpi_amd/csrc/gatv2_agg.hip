// GATv2 attention + aggregation (dgl 0.9.1 GATv2Conv.forward after fc_src / fc_dst / res_fc) and
// its atomic-free backward.  GAT's score leaky(el[u] + er[v]) needs two scalars per atom; GATv2's
//   s_e[h] = sum_f attn[h, f] * leaky(ZL[u, h, f] + ZR[v, h, f])
// needs the whole source row per edge, so these are kernels of their own beside gat_agg.hip.
//
// Column slots (all three kernels): lane l owns the float4 columns c = l + 64 j, j < NJ, of an
// H F-wide row (4 c < H F; F % 4 == 0, so a float4 never straddles two heads).  NJ in {1, 2, 3, 4, 6,
// 8} is the instance's slot count (the smallest with H F <= 256 NJ); slots past the row are masked
// (no load, no store).
// Per-head sums over a row are H per-lane partials finished with the H-value butterfly all-reduce
// (HeadReduce, wave_ops.h): a fixed shuffle tree, so every result is bitwise repeatable.
//
// Forward, one wave per destination v (xcd_block: an XCD walks one contiguous atom range):
//   sweep 1  gathers ZL[src_e] for each in-edge (2 rows in flight) and reduces s_e[h]; lane e % 64
//            keeps the scores of edge e.  An in-degree past 64 spills the raw scores to attn[e, h]
//            (the kernel's own output, rewritten below) and reads them back chunk by chunk.
//   softmax  max over the in-edges, sum of exp(s - max) in ascending slot order, a = exp / sum
//            (the arithmetic and order of gat_agg.hip's destination wave); attn[e, h] = a.
//   sweep 2  gathers the rows again (L2 hits) and sums a_e ZL[src_e] in slot order from 0, adds R,
//            applies ELU (mode 0) or the head mean (mode 1: through the wave's LDS row, heads
//            summed in order, / H, + R) and writes out[v] once.
// Backward A, one wave per contiguous range of destinations (gatv2_partial_rows(N) ranges):
//   g_a[e, h] = <ZL[u], g_rst[v]>_h; g_s = a (g_a - sum_in(v) a g_a) -> workspace [E, H];
//   gZR[v] = sum_in(v) d_e, d_e[h, f] = g_s[e, h] attn[h, f] leaky'(p_e[h, f]); gR[v] = g_rst[v]
//   (mode 1: g_out[v], F wide); the wave's running sum of g_s[e, h] leaky(p_e[h, f]) over its
//   atoms, in atom and slot order, is one row of the g_attn partials (mvml_colsum_f32 finishes).
// Backward B, one wave per source u: walks u's out-edges (out_inslot maps each to its in-CSR slot
//   for a and g_s), gathers g_rst[w] and ZR[w], and writes
//   gZL[u] = sum_out(u) (a_e g_rst[w] + d_e) once.
// No float atomics anywhere; LeakyReLU' at exactly 0 is `slope` (p > 0 ? 1 : slope).
#include "common.h"
#include "wave_ops.h"

namespace mvml {
namespace {

__device__ __forceinline__ float dleaky(float x, float slope) { return x > 0.f ? 1.f : slope; }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float4 leaky4(float4 p, float s) {
  return make_float4(leaky(p.x, s), leaky(p.y, s), leaky(p.z, s), leaky(p.w, s));
}
__device__ __forceinline__ float4 dleaky4(float4 p, float s) {
  return make_float4(dleaky(p.x, s), dleaky(p.y, s), dleaky(p.z, s), dleaky(p.w, s));
}

// The column slots of one lane.
template <int NJ>
struct Slots {
  bool ok[NJ];
  int hc[NJ];  // head of slot j
  int cz[NJ];  // float offset of slot j in a row
  __device__ __forceinline__ Slots(int lane, int HF, int F) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = 4 * (lane + 64 * j);
      ok[j] = c < HF;
      cz[j] = ok[j] ? c : 0;
      hc[j] = cz[j] / F;
    }
  }
  __device__ __forceinline__ void load(float4 (&z)[NJ], const float* row) const {
#pragma unroll
    for (int j = 0; j < NJ; ++j) z[j] = ok[j] ? ld4(row + cz[j]) : f4(0.f);
  }
  __device__ __forceinline__ void store(float* row, const float4 (&z)[NJ]) const {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (ok[j]) st4(row + cz[j], z[j]);
  }
};

// per-head <x, y> of two rows held in slots, on every lane
template <int H, int NJ>
__device__ __forceinline__ void head_dots(const Slots<NJ>& sl, const float4 (&x)[NJ], const float4 (&y)[NJ],
                                          float (&d)[H], int lane) {
#pragma unroll
  for (int h = 0; h < H; ++h) d[h] = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) add_at<H>(d, sl.hc[j], dot4(x[j], y[j]));  // masked slots hold zeros
  HeadReduce<H>::template all<false>(d, lane);
}

// sum over the first cnt lanes, in lane order, of H per-lane values, added onto acc
template <int H>
__device__ __forceinline__ void ordered_sum(const float (&p)[H], int cnt, float (&acc)[H]) {
  for (int i = 0; i < cnt; ++i)
#pragma unroll
    for (int h = 0; h < H; ++h) acc[h] += rl(p[h], i);
}

template <int H>
__device__ __forceinline__ void ld_heads(float (&a)[H], const float* p, bool in, float fill) {
  if constexpr (H == 4) {
    const float4 t = in ? ld4(p) : f4(fill);
    a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
  } else {
#pragma unroll
    for (int h = 0; h < H; ++h) a[h] = in ? p[h] : fill;
  }
}
template <int H>
__device__ __forceinline__ void st_heads(float* p, const float (&a)[H]) {
  if constexpr (H == 4) {
    st4(p, make_float4(a[0], a[1], a[2], a[3]));
  } else {
#pragma unroll
    for (int h = 0; h < H; ++h) p[h] = a[h];
  }
}

// ------------------------------------------------------------------------------------ forward
template <int H, int NJ, bool MEAN>
__global__ void __launch_bounds__(256)
gatv2_fwd_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ in_src,
                 const float* __restrict__ ZL, int64_t ldl, const float* __restrict__ ZR, int64_t ldzr,
                 const float* __restrict__ avec, const float* __restrict__ R, int64_t ldr, int F,
                 float slope, int mode, float* __restrict__ out, float* attn) {
  __shared__ __attribute__((aligned(16))) float s_rows[MEAN ? 4 * NJ * 256 : 4];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t v = xcd_block(blockIdx.x, gridDim.x) * 4 + wv;
  if (v >= N) return;  // (no block-wide barrier below)
  const int HF = H * F;
  const Slots<NJ> sl(lane, HF, F);
  float4 zr[NJ], av[NJ], acc[NJ];
  sl.load(zr, ZR + v * ldzr);
  sl.load(av, avec);
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = f4(0.f);
  const int eb = rowptr[v], deg = rowptr[v + 1] - eb;
  const bool spill = deg > 64;
  float s_l[H];  // scores of the in-edge on this lane (the last chunk swept)
  int src0 = 0;
#pragma unroll
  for (int h = 0; h < H; ++h) s_l[h] = -INFINITY;
  // sweep 1: the scores
  for (int base = 0; base < deg; base += 64) {
    const int cnt = min(64, deg - base);
    const int src_l = lane < cnt ? in_src[eb + base + lane] : 0;
    if (base == 0) src0 = src_l;
#pragma unroll
    for (int h = 0; h < H; ++h) s_l[h] = -INFINITY;
    for (int i = 0; i < cnt; i += 2) {
      float4 z[2][NJ];
#pragma unroll
      for (int u = 0; u < 2; ++u)  // past the chunk: a duplicate row, not used
        sl.load(z[u], ZL + (int64_t)rl(src_l, min(i + u, cnt - 1)) * ldl);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (i + u < cnt) {  // (uniform)
          float4 t[NJ];
#pragma unroll
          for (int j = 0; j < NJ; ++j) t[j] = leaky4(add4(z[u][j], zr[j]), slope);
          float d[H];
          head_dots<H, NJ>(sl, av, t, d, lane);
#pragma unroll
          for (int h = 0; h < H; ++h) s_l[h] = (lane == i + u) ? d[h] : s_l[h];
        }
      }
    }
    if (spill && lane < cnt) st_heads<H>(attn + (int64_t)(eb + base + lane) * H, s_l);
  }
  if (spill) wave_sync_workgroup_scope();
  // the scores of chunk `base` on the lanes (-inf past the row)
  auto scores = [&](int base, float (&s)[H]) __attribute__((always_inline)) {
    float t[H];
    if (spill) ld_heads<H>(t, attn + (int64_t)(eb + base + lane) * H, base + lane < deg, -INFINITY);
#pragma unroll
    for (int h = 0; h < H; ++h) s[h] = spill ? t[h] : s_l[h];
  };
  float m[H], sum[H];
#pragma unroll
  for (int h = 0; h < H; ++h) { m[h] = -INFINITY; sum[h] = 0.f; }
  for (int base = 0; base < deg; base += 64) {
    float s[H];
    scores(base, s);
#pragma unroll
    for (int h = 0; h < H; ++h) m[h] = fmaxf(m[h], s[h]);
  }
  HeadReduce<H>::template all<true>(m, lane);
  for (int base = 0; base < deg; base += 64) {
    float s[H], p[H];
    scores(base, s);
#pragma unroll
    for (int h = 0; h < H; ++h) p[h] = base + lane < deg ? expf(s[h] - m[h]) : 0.f;
    ordered_sum<H>(p, min(64, deg - base), sum);
  }
  // sweep 2: the attention and the weighted sum of the source rows
  for (int base = 0; base < deg; base += 64) {
    const int cnt = min(64, deg - base);
    const int src_l = base == 0 ? src0 : (lane < cnt ? in_src[eb + base + lane] : 0);
    float s[H], a_l[H];
    scores(base, s);
#pragma unroll
    for (int h = 0; h < H; ++h) a_l[h] = lane < cnt ? expf(s[h] - m[h]) / sum[h] : 0.f;
    if (lane < cnt) st_heads<H>(attn + (int64_t)(eb + base + lane) * H, a_l);
    for (int i = 0; i < cnt; i += 2) {
      float4 z[2][NJ];
#pragma unroll
      for (int u = 0; u < 2; ++u) sl.load(z[u], ZL + (int64_t)rl(src_l, min(i + u, cnt - 1)) * ldl);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (i + u < cnt) {
          HeadVals<H> a;
#pragma unroll
          for (int h = 0; h < H; ++h) a.v[h] = rl(a_l[h], i + u);
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[j] = fma4(pick<H>(a, sl.hc[j]), z[u][j], acc[j]);
        }
      }
    }
  }
  if constexpr (MEAN) {
    float* row = s_rows + wv * (NJ * 256);
    sl.store(row, acc);
    wave_sync_workgroup_scope();
    const float* rv = R ? R + v * ldr : nullptr;
    const float invh = (float)H;
    for (int q = 4 * lane; q < F; q += 256) {
      float4 tot = ld4(row + q);
      for (int h = 1; h < H; ++h) tot = add4(tot, ld4(row + h * F + q));
      const float4 r = rv ? ld4(rv + q) : f4(0.f);
      st4(out + v * F + q, make_float4(tot.x / invh + r.x, tot.y / invh + r.y, tot.z / invh + r.z,
                                       tot.w / invh + r.w));
    }
  } else {
    if (R) {
      float4 r[NJ];
      sl.load(r, R + v * ldr);
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = add4(acc[j], r[j]);
    }
    if (mode == 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = make_float4(elu(acc[j].x), elu(acc[j].y), elu(acc[j].z), elu(acc[j].w));
    }
    sl.store(out + v * HF, acc);
  }
}

// ---------------------------------------------------------------------- backward A (by destination)
template <int H, int NJ>
__global__ void __launch_bounds__(256)
gatv2_bwd_dst_kernel(int64_t N, int64_t apw, const int32_t* __restrict__ rowptr,
                     const int32_t* __restrict__ in_src, const float* __restrict__ ZL, int64_t ldl,
                     const float* __restrict__ ZR, int64_t ldzr, const float* __restrict__ avec,
                     const float* __restrict__ attn, const float* __restrict__ out,
                     const float* __restrict__ g_out, int F, float slope, int mode, float* gs,
                     float* __restrict__ gZR, int64_t ldgzr, float* __restrict__ gR, int64_t ldgr,
                     float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t v0 = wid * apw, v1 = min(N, v0 + apw);
  if (v0 >= N) return;
  const int HF = H * F;
  const Slots<NJ> sl(lane, HF, F);
  float4 av[NJ], gat[NJ];
  sl.load(av, avec);
#pragma unroll
  for (int j = 0; j < NJ; ++j) gat[j] = f4(0.f);
  for (int64_t v = v0; v < v1; ++v) {
    // (g_rst[v] is live across sweep 1 only and ZR[v] across sweep 2 only: the gR store below
    // forms g_rst again from rows that are in cache, 4 NJ fewer registers held through sweep 2)
    float4 g[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) g[j] = sl.ok[j] ? grst_of(g_out, out, v, sl.cz[j], HF, F, H, mode) : f4(0.f);
    const int eb = rowptr[v], deg = rowptr[v + 1] - eb;
    const bool spill = deg > 64;
    float ga_l[H], dot[H];
    int src0 = 0;
#pragma unroll
    for (int h = 0; h < H; ++h) { ga_l[h] = 0.f; dot[h] = 0.f; }
    // sweep 1: g_a[e, h] on the lanes, and sum_e a g_a in slot order
    for (int base = 0; base < deg; base += 64) {
      const int cnt = min(64, deg - base);
      const int src_l = lane < cnt ? in_src[eb + base + lane] : 0;
      if (base == 0) src0 = src_l;
#pragma unroll
      for (int h = 0; h < H; ++h) ga_l[h] = 0.f;
      for (int i = 0; i < cnt; i += 2) {
        float4 z[2][NJ];
#pragma unroll
        for (int u = 0; u < 2; ++u) sl.load(z[u], ZL + (int64_t)rl(src_l, min(i + u, cnt - 1)) * ldl);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (i + u < cnt) {
            float d[H];
            head_dots<H, NJ>(sl, z[u], g, d, lane);
#pragma unroll
            for (int h = 0; h < H; ++h) ga_l[h] = (lane == i + u) ? d[h] : ga_l[h];
          }
        }
      }
      float a_l[H], t[H];
      ld_heads<H>(a_l, attn + (int64_t)(eb + base + lane) * H, lane < cnt, 0.f);
#pragma unroll
      for (int h = 0; h < H; ++h) t[h] = a_l[h] * ga_l[h];
      ordered_sum<H>(t, cnt, dot);
      if (spill && lane < cnt) st_heads<H>(gs + (int64_t)(eb + base + lane) * H, ga_l);
    }
    if (spill) wave_sync_workgroup_scope();
    // sweep 2: g_s, gZR[v] and the g_attn partial
    float4 zr[NJ], gzr[NJ];
    sl.load(zr, ZR + v * ldzr);
#pragma unroll
    for (int j = 0; j < NJ; ++j) gzr[j] = f4(0.f);
    for (int base = 0; base < deg; base += 64) {
      const int cnt = min(64, deg - base);
      const int src_l = base == 0 ? src0 : (lane < cnt ? in_src[eb + base + lane] : 0);
      float a_l[H], gs_l[H];
      ld_heads<H>(a_l, attn + (int64_t)(eb + base + lane) * H, lane < cnt, 0.f);
      if (spill) ld_heads<H>(ga_l, gs + (int64_t)(eb + base + lane) * H, lane < cnt, 0.f);
#pragma unroll
      for (int h = 0; h < H; ++h) gs_l[h] = a_l[h] * (ga_l[h] - dot[h]);
      if (lane < cnt) st_heads<H>(gs + (int64_t)(eb + base + lane) * H, gs_l);
      for (int i = 0; i < cnt; i += 2) {
        float4 z[2][NJ];
#pragma unroll
        for (int u = 0; u < 2; ++u) sl.load(z[u], ZL + (int64_t)rl(src_l, min(i + u, cnt - 1)) * ldl);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (i + u < cnt) {
            HeadVals<H> s;
#pragma unroll
            for (int h = 0; h < H; ++h) s.v[h] = rl(gs_l[h], i + u);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
              const float4 p = add4(z[u][j], zr[j]);
              const float sj = pick<H>(s, sl.hc[j]);
              gzr[j] = fma4(sj, mul4(av[j], dleaky4(p, slope)), gzr[j]);
              gat[j] = fma4(sj, leaky4(p, slope), gat[j]);
            }
          }
        }
      }
    }
    sl.store(gZR + v * ldgzr, gzr);
    if (gR) {
      if (mode == 1) {  // the head-mean residual's gradient is g_out itself (F wide)
        for (int q = 4 * lane; q < F; q += 256) st4(gR + v * ldgr + q, ld4(g_out + v * F + q));
      } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          if (sl.ok[j]) st4(gR + v * ldgr + sl.cz[j], grst_of(g_out, out, v, sl.cz[j], HF, F, H, mode));
      }
    }
  }
  sl.store(part + wid * HF, gat);
}

// --------------------------------------------------------------------------- backward B (by source)
template <int H, int NJ>
__global__ void __launch_bounds__(256)
gatv2_bwd_src_kernel(int64_t N, const int32_t* __restrict__ out_rowptr, const int32_t* __restrict__ out_dst,
                     const int32_t* __restrict__ out_inslot, const float* __restrict__ ZL, int64_t ldl,
                     const float* __restrict__ ZR, int64_t ldzr, const float* __restrict__ avec,
                     const float* __restrict__ attn, const float* __restrict__ gs,
                     const float* __restrict__ out, const float* __restrict__ g_out, int F, float slope,
                     int mode, float* __restrict__ gZL, int64_t ldgzl) {
  const int lane = threadIdx.x & 63;
  const int64_t u = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (u >= N) return;
  const int HF = H * F;
  const Slots<NJ> sl(lane, HF, F);
  float4 av[NJ], zl[NJ], acc[NJ];
  sl.load(av, avec);
  sl.load(zl, ZL + u * ldl);
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = f4(0.f);
  const int ob = out_rowptr[u], od = out_rowptr[u + 1] - ob;
  for (int base = 0; base < od; base += 64) {
    const int cnt = min(64, od - base);
    const bool in = lane < cnt;
    const int w_l = in ? out_dst[ob + base + lane] : 0;
    const int slot = in ? out_inslot[ob + base + lane] : 0;
    float a_l[H], gs_l[H];
    ld_heads<H>(a_l, attn + (int64_t)slot * H, in, 0.f);
    ld_heads<H>(gs_l, gs + (int64_t)slot * H, in, 0.f);
    // one out-edge in flight: two (ZR[w] and g_rst[w] rows of both held at once) cost a wave per
    // SIMD at NJ >= 3 and measured 6 % (4 x 192) to 24 % (4 x 384) slower
    for (int i = 0; i < cnt; ++i) {
      const int64_t w = rl(w_l, i);
      float4 zr[NJ], g[NJ];
      sl.load(zr, ZR + w * ldzr);
#pragma unroll
      for (int j = 0; j < NJ; ++j) g[j] = sl.ok[j] ? grst_of(g_out, out, w, sl.cz[j], HF, F, H, mode) : f4(0.f);
      HeadVals<H> a, s;
#pragma unroll
      for (int h = 0; h < H; ++h) { a.v[h] = rl(a_l[h], i); s.v[h] = rl(gs_l[h], i); }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float4 p = add4(zl[j], zr[j]);
        acc[j] = fma4(pick<H>(a, sl.hc[j]), g[j], acc[j]);
        acc[j] = fma4(pick<H>(s, sl.hc[j]), mul4(av[j], dleaky4(p, slope)), acc[j]);
      }
    }
  }
  sl.store(gZL + u * ldgzl, acc);
}

__global__ void __launch_bounds__(256)
add_cols_kernel(int64_t rows, int c4, const float* __restrict__ src, int64_t lds, float* __restrict__ dst,
                int64_t ldd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * c4) return;
  const int64_t r = i / c4;
  const int c = 4 * (int)(i % c4);
  st4(dst + r * ldd + c, add4(ld4(dst + r * ldd + c), ld4(src + r * lds + c)));
}

// Two [N, HF] column blocks (row strides lda, ldb) that share no element: apart as whole ranges,
// or at one pitch with column ranges that do not meet.
bool blocks_disjoint(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t N, int64_t HF) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  const int64_t d = (int64_t)((pa < pb ? pb - pa : pa - pb) / sizeof(float));
  const int64_t ldlo = pa < pb ? lda : ldb;
  if (d >= (std::max<int64_t>(N, 1) - 1) * ldlo + HF) return true;
  if (lda != ldb) return false;
  const int64_t c = d % lda;
  return c >= HF && c + HF <= lda;
}

int check_shapes(int H, int F, int mode, const char* who) {
  if (int rc = check_heads(H, F, who)) return rc;
  MVML_REQUIRE(mode >= 0 && mode <= 2, "%s: mode must be 0, 1 or 2 (got %d)", who, mode);
  return MVML_OK;
}

int slots_of(int HF) { return HF <= 1024 ? (HF + 255) / 256 : HF <= 1536 ? 6 : 8; }

// Destinations per wave of backward A: the g_attn partials are gatv2_partial_rows(N) rows, a
// function of N alone (at most 32768 rows of H F floats, whatever N: under 2 % of one read of Z
// at the bench batches).
int64_t atoms_per_wave(int64_t N) { return std::max<int64_t>(16, ceil_div(N, 32768)); }

struct FwdArgs {
  int64_t N;
  const int32_t *rowptr, *in_src;
  const float *ZL, *ZR, *avec, *R;
  int64_t ldl, ldzr, ldr;
  int F;
  float slope;
  int mode;
  float *out, *attn;
};

template <int H, int NJ>
int launch_fwd(const FwdArgs& a, hipStream_t st) {
  const unsigned blocks = (unsigned)ceil_div(a.N, 4);
  if (a.mode == 1)
    gatv2_fwd_kernel<H, NJ, true><<<blocks, 256, 0, st>>>(a.N, a.rowptr, a.in_src, a.ZL, a.ldl, a.ZR, a.ldzr,
                                                          a.avec, a.R, a.ldr, a.F, a.slope, a.mode, a.out, a.attn);
  else
    gatv2_fwd_kernel<H, NJ, false><<<blocks, 256, 0, st>>>(a.N, a.rowptr, a.in_src, a.ZL, a.ldl, a.ZR, a.ldzr,
                                                           a.avec, a.R, a.ldr, a.F, a.slope, a.mode, a.out, a.attn);
  return check_launch("gatv2_fwd_kernel");
}

struct BwdArgs {
  int64_t N;
  const int32_t *rowptr, *in_src, *out_rowptr, *out_dst, *out_inslot;
  const float *ZL, *ZR, *avec, *attn, *out, *g_out;
  int64_t ldl, ldzr;
  int F;
  float slope;
  int mode;
  float *gs, *gZL, *gZR, *gR, *part;
  int64_t ldgzl, ldgzr, ldgr;
};

template <int H, int NJ>
int launch_bwd(const BwdArgs& a, hipStream_t st) {
  const int64_t apw = atoms_per_wave(a.N);
  const unsigned blocks_a = (unsigned)ceil_div(ceil_div(a.N, apw), 4);
  gatv2_bwd_dst_kernel<H, NJ><<<blocks_a, 256, 0, st>>>(a.N, apw, a.rowptr, a.in_src, a.ZL, a.ldl, a.ZR, a.ldzr,
                                                        a.avec, a.attn, a.out, a.g_out, a.F, a.slope, a.mode,
                                                        a.gs, a.gZR, a.ldgzr, a.gR, a.ldgr, a.part);
  int rc = check_launch("gatv2_bwd_dst_kernel");
  if (rc) return rc;
  gatv2_bwd_src_kernel<H, NJ><<<(unsigned)ceil_div(a.N, 4), 256, 0, st>>>(
      a.N, a.out_rowptr, a.out_dst, a.out_inslot, a.ZL, a.ldl, a.ZR, a.ldzr, a.avec, a.attn, a.gs, a.out,
      a.g_out, a.F, a.slope, a.mode, a.gZL, a.ldgzl);
  return check_launch("gatv2_bwd_src_kernel");
}

// launch(h, nj), as std::integral_constant values, for the instance of this shape
template <typename Fn>
int dispatch(int H, int F, const char* who, Fn&& launch) {
  const int rc = switch_const<1, 2, 4, 8>(H, [&](auto h) {
    return switch_const<1, 2, 3, 4, 6, 8>(slots_of(H * F), [&](auto nj) { return launch(h, nj); });
  });
  if (rc != kNoCase) return rc;
  set_error("%s: unsupported shape", who);
  return MVML_ERR_INVALID;
}
int dispatch_fwd(int H, int F, const FwdArgs& a, hipStream_t st) {
  return dispatch(H, F, "gatv2_agg_fwd",
                  [&](auto h, auto nj) { return launch_fwd<decltype(h)::value, decltype(nj)::value>(a, st); });
}
int dispatch_bwd(int H, int F, const BwdArgs& a, hipStream_t st) {
  return dispatch(H, F, "gatv2_agg_bwd",
                  [&](auto h, auto nj) { return launch_bwd<decltype(h)::value, decltype(nj)::value>(a, st); });
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int64_t mvml_gatv2_partial_rows(int64_t num_nodes) {
  return num_nodes <= 0 ? 0 : ceil_div(num_nodes, atoms_per_wave(num_nodes));
}

extern "C" int mvml_gatv2_agg_fwd(int64_t num_nodes, const int32_t* in_rowptr, const int32_t* in_src,
                                  const float* ZL, int64_t ldzl, const float* ZR, int64_t ldzr, int H, int F,
                                  const float* attn_vec, const float* R, int64_t ldr, float slope, int mode,
                                  float* out, float* attn, void* stream) {
  clear_error();
  int rc = check_shapes(H, F, mode, "gatv2_agg_fwd");
  if (rc) return rc;
  const int HF = H * F, RW = mode == 1 ? F : HF;
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "gatv2_agg_fwd: num_nodes out of range");
  MVML_REQUIRE(row_ok(ZL, ldzl, HF) && row_ok(ZR, ldzr, HF),
               "gatv2_agg_fwd: ZL / ZR must be 16-byte aligned with row strides >= %d that are multiples of 4", HF);
  MVML_REQUIRE(R == nullptr || row_ok(R, ldr, RW),
               "gatv2_agg_fwd: R must be 16-byte aligned with a row stride ldr >= %d that is a multiple of 4", RW);
  MVML_REQUIRE(attn_vec && aligned16(attn_vec) && out && aligned16(out) && attn && aligned16(attn),
               "gatv2_agg_fwd: attn_vec, out and attn are required, 16-byte aligned");
  MVML_REQUIRE(in_rowptr && (in_src || num_nodes == 0), "gatv2_agg_fwd: the in-CSR is required");
  if (num_nodes == 0) return MVML_OK;
  const FwdArgs a{num_nodes, in_rowptr, in_src, ZL, ZR, attn_vec, R, ldzl, ldzr, ldr, F, slope, mode, out, attn};
  return dispatch_fwd(H, F, a, as_stream(stream));
}

extern "C" size_t mvml_gatv2_agg_bwd_workspace_size(int64_t num_nodes, int64_t num_edges, int H, int F) {
  const int64_t P = mvml_gatv2_partial_rows(num_nodes);
  return carve_size((size_t)std::max<int64_t>(num_edges, 1) * H * sizeof(float)) +
         carve_size((size_t)std::max<int64_t>(P, 1) * H * F * sizeof(float)) +
         carve_size(mvml_colsum_workspace_size(P, (int64_t)H * F)) + 256;
}

extern "C" int mvml_gatv2_agg_bwd(int64_t num_nodes, const int32_t* in_rowptr, const int32_t* in_src,
                                  const int32_t* out_rowptr, const int32_t* out_dst, const int32_t* out_inslot,
                                  int64_t num_edges, const float* ZL, int64_t ldzl, const float* ZR,
                                  int64_t ldzr, int H, int F, const float* attn_vec, const float* attn,
                                  const float* out, const float* g_out, float slope, int mode, float* gZL,
                                  int64_t ldgzl, float* gZR, int64_t ldgzr, float* gR, int64_t ldgr,
                                  float* g_attn_vec, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  int rc = check_shapes(H, F, mode, "gatv2_agg_bwd");
  if (rc) return rc;
  const int HF = H * F, RW = mode == 1 ? F : HF;
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31) && num_edges >= 0,
               "gatv2_agg_bwd: num_nodes / num_edges out of range");
  MVML_REQUIRE(row_ok(ZL, ldzl, HF) && row_ok(ZR, ldzr, HF),
               "gatv2_agg_bwd: ZL / ZR must be 16-byte aligned with row strides >= %d that are multiples of 4", HF);
  MVML_REQUIRE(row_ok(gZL, ldgzl, HF) && row_ok(gZR, ldgzr, HF) &&
                   blocks_disjoint(gZL, ldgzl, gZR, ldgzr, num_nodes, HF),
               "gatv2_agg_bwd: gZL / gZR must be two 16-byte aligned outputs with row strides >= %d that are "
               "multiples of 4", HF);
  MVML_REQUIRE(gR == nullptr || row_ok(gR, ldgr, RW),
               "gatv2_agg_bwd: gR must be 16-byte aligned with a row stride ldgr >= %d that is a multiple of 4", RW);
  MVML_REQUIRE(attn_vec && aligned16(attn_vec) && attn && aligned16(attn) && g_out && aligned16(g_out) &&
                   g_attn_vec && (mode != 0 || (out && aligned16(out))),
               "gatv2_agg_bwd: attn_vec, attn, g_out (and out in mode 0) are required, 16-byte aligned");
  MVML_REQUIRE(in_rowptr && out_rowptr && ((in_src && out_dst && out_inslot) || num_edges == 0),
               "gatv2_agg_bwd: both CSRs are required");
  if (num_nodes == 0) return MVML_OK;
  if (workspace_bytes < mvml_gatv2_agg_bwd_workspace_size(num_nodes, num_edges, H, F) || !workspace) {
    set_error("gatv2_agg_bwd: workspace too small");
    return MVML_ERR_WORKSPACE;
  }
  const int64_t P = mvml_gatv2_partial_rows(num_nodes);
  Carver cv(workspace, workspace_bytes);
  float* gs = cv.take<float>((size_t)std::max<int64_t>(num_edges, 1) * H);
  float* part = cv.take<float>((size_t)P * HF);
  const size_t csz = mvml_colsum_workspace_size(P, HF);
  char* cws = cv.take<char>(csz);
  const BwdArgs a{num_nodes, in_rowptr, in_src, out_rowptr, out_dst, out_inslot, ZL, ZR, attn_vec, attn, out,
                  g_out, ldzl, ldzr, F, slope, mode, gs, gZL, gZR, gR, part, ldgzl, ldgzr, ldgr};
  rc = dispatch_bwd(H, F, a, as_stream(stream));
  if (rc) return rc;
  return mvml_colsum_f32(P, HF, part, HF, 1.f, 0.f, g_attn_vec, csz ? cws : nullptr, csz, stream);
}

extern "C" int mvml_add_cols_f32(int64_t rows, int cols, const float* src, int64_t lds, float* dst, int64_t ldd,
                                 void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && cols > 0 && cols % 4 == 0 && row_ok(src, lds, cols) && row_ok(dst, ldd, cols),
               "add_cols: 16-byte aligned rows of a multiple of 4 columns");
  if (rows == 0) return MVML_OK;
  add_cols_kernel<<<(unsigned)ceil_div(rows * (cols / 4), 256), 256, 0, as_stream(stream)>>>(rows, cols / 4, src, lds,
                                                                                            dst, ldd);
  return check_launch("add_cols_kernel");
}
