// SAGEConv's aggregations that mvml_gcn_agg does not cover (dgl 0.9.1 SAGEConv.forward):
//
//   pool:  out[v, c] = max_s X[nbr[s], c]          s over v's in-CSR row, arg[v, c] the in-CSR slot
//          gX[u, c]  = sum_t [arg[dst[t], c] == inslot[t]] G[dst[t], c]     t over u's out-CSR row
//   gcn:   s[v] = 1 / (in_degree(v) + 1),  out[v] += s[v] * X[v]  (the self term; its own adjoint)
//
// (mean and the neighbour sum of gcn are mvml_gcn_agg with a row scale.)
//
// The two maximum kernels have gcn_agg_row_kernel's form (gcn_agg.hip): one wave per row
// (xcd_block), lanes on the float4 columns c = lane + 64 j with the last slot masked, the ids
// loaded 64 per chunk onto the lanes and broadcast by readlane, whole neighbour rows gathered into
// registers (U in flight), one non-temporal store per output row.  The forward keeps, per element,
// the running maximum and the global in-CSR slot that first attained it (strict >, so the first
// maximiser in row order wins a tie); a maximum rounds nothing, so a row's bits depend on neither
// the instance, the chunking nor the batch.  The backward is a gather over the out-CSR: out-edge t
// of u hands G[dst[t], c] to gX[u, c] where dst[t]'s argmax is this very edge's in-slot (the slot
// is compared, not the source id: of two parallel edges only the first receives), added in slot
// order from 0 with __fadd_rn.  No atomics, no LDS except block_amax_commit's 16 bytes.
//
// Narrow rows (D <= 64) run four to a wave in the sub-wave forms below, bitwise the one-row forms;
// MVML_OPT_SAGE_SUBWAVE picks the form for D <= 64.
#include "gat_agg_common.h"

namespace mvml {
namespace {

typedef int mvml_i4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int4 ldi4(const int32_t* p) { return *reinterpret_cast<const int4*>(p); }
__device__ __forceinline__ void sti4nt(int32_t* p, int4 v) {
  mvml_i4v w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<mvml_i4v*>(p));
}
// one element of the running maximum: the first slot of a row always enters, later ones on >
__device__ __forceinline__ void max_step(float x, int slot, bool first, float& m, int& a) {
  const bool up = first || x > m;
  m = up ? x : m;
  a = up ? slot : a;
}

// One wave per row; NJ float4 column slots per lane, U neighbour rows in flight.
template <int NJ, int U>
__global__ void __launch_bounds__(256)
sage_max_fwd_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
                    const float* __restrict__ X, int64_t ldx, int D, float* __restrict__ out, int64_t ldo,
                    int32_t* __restrict__ arg, int64_t lda, uint32_t* __restrict__ out_amax,
                    uint32_t* __restrict__ out_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t v = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float omx = 0.f;
  if (v < N) {  // (no early return: block_amax_commit below has a barrier)
    bool ok[NJ];
    float4 mx[NJ];
    int4 am[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      ok[j] = 4 * (lane + 64 * j) < D;
      mx[j] = f4(0.f);  // a row without entries: 0 and -1
      am[j] = make_int4(-1, -1, -1, -1);
    }
    const int eb = rowptr[v], deg = rowptr[v + 1] - eb;
    for (int base = 0; base < deg; base += 64) {  // more than 64 entries (hubs): more chunks
      const int cnt = min(64, deg - base);
      const int id_l = lane < cnt ? nbr[eb + base + lane] : 0;
      for (int j0 = 0; j0 < cnt; j0 += U) {
        float4 x[U][NJ];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = min(j0 + u, cnt - 1);  // past the chunk: a duplicate row, not compared
          const float* xr = X + (int64_t)rl(id_l, e) * ldx;
#pragma unroll
          for (int j = 0; j < NJ; ++j) x[u][j] = ok[j] ? ld4(xr + 4 * (lane + 64 * j)) : f4(0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (j0 + u < cnt) {  // (uniform)
            const int slot = eb + base + j0 + u;
            const bool first = base + j0 + u == 0;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
              max_step(x[u][j].x, slot, first, mx[j].x, am[j].x);
              max_step(x[u][j].y, slot, first, mx[j].y, am[j].y);
              max_step(x[u][j].z, slot, first, mx[j].z, am[j].z);
              max_step(x[u][j].w, slot, first, mx[j].w, am[j].w);
            }
          }
        }
      }
    }
    float rmx = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (!ok[j]) continue;
      const int c = 4 * (lane + 64 * j);
      st4nt(out + v * ldo + c, mx[j]);
      sti4nt(arg + v * lda + c, am[j]);
      rmx = amax4(rmx, mx[j]);
    }
    omx = wave_max(rmx);
    if (out_rows && lane == 0) out_rows[v] = __float_as_uint(omx);
  }
  if (out_amax) block_amax_commit<256>(omx, out_amax);
}

__device__ __forceinline__ float4 take4(float4 acc, float4 g, int4 a, int slot) {
  return make_float4(__fadd_rn(acc.x, a.x == slot ? g.x : 0.f), __fadd_rn(acc.y, a.y == slot ? g.y : 0.f),
                     __fadd_rn(acc.z, a.z == slot ? g.z : 0.f), __fadd_rn(acc.w, a.w == slot ? g.w : 0.f));
}

// One wave per source row u over the out-CSR; the destination ids and the edges' in-slots ride
// on the lanes, 64 per chunk.
template <int NJ, int U>
__global__ void __launch_bounds__(256)
sage_max_bwd_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ dst,
                    const int32_t* __restrict__ inslot, const float* __restrict__ G, int64_t ldg,
                    const int32_t* __restrict__ arg, int64_t lda, int D, const float* __restrict__ P,
                    int64_t ldp, float* __restrict__ gX, int64_t ldgx) {
  const int lane = threadIdx.x & 63;
  const int64_t u_row = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (u_row >= N) return;
  bool ok[NJ];
  float4 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    ok[j] = 4 * (lane + 64 * j) < D;
    acc[j] = f4(0.f);
  }
  const int eb = rowptr[u_row], deg = rowptr[u_row + 1] - eb;
  for (int base = 0; base < deg; base += 64) {
    const int cnt = min(64, deg - base);
    const int id_l = lane < cnt ? dst[eb + base + lane] : 0;
    const int sl_l = lane < cnt ? inslot[eb + base + lane] : -2;
    for (int j0 = 0; j0 < cnt; j0 += U) {
      float4 g[U][NJ];
      int4 a[U][NJ];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = min(j0 + u, cnt - 1);  // past the chunk: a duplicate row, not added
        const int64_t w = rl(id_l, e);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = 4 * (lane + 64 * j);
          g[u][j] = ok[j] ? ld4(G + w * ldg + c) : f4(0.f);
          a[u][j] = ok[j] ? ldi4(arg + w * lda + c) : make_int4(-1, -1, -1, -1);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (j0 + u < cnt) {  // (uniform)
          const int slot = rl(sl_l, j0 + u);
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[j] = take4(acc[j], g[u][j], a[u][j], slot);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (!ok[j]) continue;
    const int c = 4 * (lane + 64 * j);
    float4 o = acc[j];
    if (P) {  // the ReLU whose output was pooled: its gradient passes where that output is > 0
      const float4 p = ld4(P + u_row * ldp + c);
      o = make_float4(p.x > 0.f ? o.x : 0.f, p.y > 0.f ? o.y : 0.f, p.z > 0.f ? o.z : 0.f, p.w > 0.f ? o.w : 0.f);
    }
    st4nt(gX + u_row * ldgx + c, o);
  }
}

// Sub-wave forms, D <= 64 (gcn_agg_sub_kernel's shape): each 16-lane group of a wave owns one row
// (16 rows per workgroup), lane s of a group the float4 column s, the ids on the group's lanes 16
// per chunk.  The chunk loops run to the wave's longest row; a group past its own row's end loads
// and compares nothing.  The same comparisons / additions in the same order as the one-row forms:
// the same bits.
__device__ __forceinline__ int groups_max(int x) {  // over a wave's four groups, x uniform in each
  x = max(x, __shfl_xor(x, 16, 64));
  return max(x, __shfl_xor(x, 32, 64));
}

template <int U>
__global__ void __launch_bounds__(256)
sage_max_fwd_sub_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
                        const float* __restrict__ X, int64_t ldx, int D, float* __restrict__ out, int64_t ldo,
                        int32_t* __restrict__ arg, int64_t lda, uint32_t* __restrict__ out_amax,
                        uint32_t* __restrict__ out_rows) {
  const int lane = threadIdx.x & 63, sl = lane & 15, g0 = lane & 48;
  const int64_t v = (xcd_block(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const bool row = v < N;
  const bool ok = row && 4 * sl < D;
  int eb = 0, deg = 0;
  if (row) {
    eb = rowptr[v];
    deg = rowptr[v + 1] - eb;
  }
  const int mdeg = groups_max(deg);
  float4 mx = f4(0.f);
  int4 am = make_int4(-1, -1, -1, -1);
  for (int base = 0; base < mdeg; base += 16) {
    const int cnt = max(0, min(16, deg - base));
    const int id_l = sl < cnt ? nbr[eb + base + sl] : 0;
    const int mcnt = groups_max(cnt);
    for (int j0 = 0; j0 < mcnt; j0 += U) {
      float4 x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int id = __shfl(id_l, g0 + min(j0 + u, 15), 64);
        x[u] = (ok && j0 + u < cnt) ? ld4(X + (int64_t)id * ldx + 4 * sl) : f4(0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (j0 + u < cnt) {
          const int slot = eb + base + j0 + u;
          const bool first = base + j0 + u == 0;
          max_step(x[u].x, slot, first, mx.x, am.x);
          max_step(x[u].y, slot, first, mx.y, am.y);
          max_step(x[u].z, slot, first, mx.z, am.z);
          max_step(x[u].w, slot, first, mx.w, am.w);
        }
      }
    }
  }
  float rmx = 0.f;
  if (ok) {
    st4nt(out + v * ldo + 4 * sl, mx);
    sti4nt(arg + v * lda + 4 * sl, am);
    rmx = amax4(rmx, mx);
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) rmx = fmaxf(rmx, __shfl_xor(rmx, o, 64));  // the group's row
  if (out_rows && row && sl == 0) out_rows[v] = __float_as_uint(rmx);
  if (out_amax) block_amax_commit<256>(rmx, out_amax);
}

template <int U>
__global__ void __launch_bounds__(256)
sage_max_bwd_sub_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ dst,
                        const int32_t* __restrict__ inslot, const float* __restrict__ G, int64_t ldg,
                        const int32_t* __restrict__ arg, int64_t lda, int D, const float* __restrict__ P,
                        int64_t ldp, float* __restrict__ gX, int64_t ldgx) {
  const int lane = threadIdx.x & 63, sl = lane & 15, g0 = lane & 48;
  const int64_t u_row = (xcd_block(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const bool row = u_row < N;
  const bool ok = row && 4 * sl < D;
  int eb = 0, deg = 0;
  if (row) {
    eb = rowptr[u_row];
    deg = rowptr[u_row + 1] - eb;
  }
  const int mdeg = groups_max(deg);
  float4 acc = f4(0.f);
  for (int base = 0; base < mdeg; base += 16) {
    const int cnt = max(0, min(16, deg - base));
    const int id_l = sl < cnt ? dst[eb + base + sl] : 0;
    const int sl_l = sl < cnt ? inslot[eb + base + sl] : -2;
    const int mcnt = groups_max(cnt);
    for (int j0 = 0; j0 < mcnt; j0 += U) {
      float4 g[U];
      int4 a[U];
      int slot[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = g0 + min(j0 + u, 15);
        const int64_t w = __shfl(id_l, e, 64);
        slot[u] = __shfl(sl_l, e, 64);
        const bool live = ok && j0 + u < cnt;
        g[u] = live ? ld4(G + w * ldg + 4 * sl) : f4(0.f);
        a[u] = live ? ldi4(arg + w * lda + 4 * sl) : make_int4(-1, -1, -1, -1);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j0 + u < cnt) acc = take4(acc, g[u], a[u], slot[u]);
    }
  }
  if (ok) {
    float4 o = acc;
    if (P) {
      const float4 p = ld4(P + u_row * ldp + 4 * sl);
      o = make_float4(p.x > 0.f ? o.x : 0.f, p.y > 0.f ? o.y : 0.f, p.z > 0.f ? o.z : 0.f, p.w > 0.f ? o.w : 0.f);
    }
    st4nt(gX + u_row * ldgx + 4 * sl, o);
  }
}

// One thread per node: 1 / (in-degree + 1), rounded once from double.
__global__ void __launch_bounds__(256)
sage_gcn_scale_kernel(int64_t N, const int32_t* __restrict__ in_rowptr, float* __restrict__ scale) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < N) scale[v] = (float)(1.0 / ((double)(in_rowptr[v + 1] - in_rowptr[v]) + 1.0));
}

// One thread per float4: out[v] = act(fma(s[v], X[v], out[v]) + bias), every step rounded once.
__global__ void __launch_bounds__(256)
sage_self_add_kernel(int64_t N, const float* __restrict__ X, int64_t ldx, int D, const float* __restrict__ s,
                     const float* __restrict__ bias, int act, float* out, int64_t ldo) {
  const int q = D / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * q) return;
  const int64_t v = i / q;
  const int c = 4 * (int)(i - v * q);
  const float sv = s[v];
  const float4 x = ld4(X + v * ldx + c), o = ld4(out + v * ldo + c);
  float4 r = make_float4(__fmaf_rn(sv, x.x, o.x), __fmaf_rn(sv, x.y, o.y), __fmaf_rn(sv, x.z, o.z),
                         __fmaf_rn(sv, x.w, o.w));
  if (bias) {
    const float4 b = ld4(bias + c);
    r = make_float4(__fadd_rn(r.x, b.x), __fadd_rn(r.y, b.y), __fadd_rn(r.z, b.z), __fadd_rn(r.w, b.w));
  }
  if (act) r = make_float4(fmaxf(r.x, 0.f), fmaxf(r.y, 0.f), fmaxf(r.z, 0.f), fmaxf(r.w, 0.f));
  st4(out + v * ldo + c, r);
}

// Neighbour rows in flight per wave, by column slots per lane (gcn_agg.hip's choice).
constexpr int sage_rows_in_flight(int NJ) { return NJ <= 2 ? 4 : 2; }

// the address ranges of the rows of a [n, D] float matrix at stride ld
inline bool rows_meet(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t n, int D) {
  const char *a0 = (const char*)a, *a1 = a0 + 4 * ((n - 1) * lda + D);
  const char *b0 = (const char*)b, *b1 = b0 + 4 * ((n - 1) * ldb + D);
  return !(a1 <= b0 || b1 <= a0);
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_sage_max_fwd(int64_t num_nodes, const int32_t* in_rowptr, const int32_t* in_src,
                                 const float* X, int64_t ldx, int D, float* out, int64_t ldo, int32_t* arg,
                                 int64_t lda, uint32_t* out_amax, uint32_t* out_row_amax, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "sage_max_fwd: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "sage_max_fwd: D must be a positive multiple of 4 <= 2048 (got %d)", D);
  MVML_REQUIRE(in_rowptr != nullptr && in_src != nullptr, "sage_max_fwd: in_rowptr and in_src are required");
  MVML_REQUIRE(row_ok(X, ldx, D) && row_ok(out, ldo, D) && row_ok(arg, lda, D),
               "sage_max_fwd: X, out and arg must be 16-byte aligned with row strides >= D that are multiples of 4");
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(!rows_meet(X, ldx, out, ldo, num_nodes, D) && !rows_meet(X, ldx, arg, lda, num_nodes, D),
               "sage_max_fwd: out and arg must not alias X");
  MVML_REQUIRE(!rows_meet(out, ldo, arg, lda, num_nodes, D), "sage_max_fwd: out and arg must not alias each other");
  const hipStream_t st = as_stream(stream);
  uint32_t* blk_amax = out_row_amax ? nullptr : out_amax;
  if (D <= 64 && option(MVML_OPT_SAGE_SUBWAVE) != 0) {
    sage_max_fwd_sub_kernel<4><<<(unsigned)ceil_div(num_nodes, 16), 256, 0, st>>>(
        num_nodes, in_rowptr, in_src, X, ldx, D, out, ldo, arg, lda, blk_amax, out_row_amax);
  } else {
    const int nj = (int)ceil_div(D / 4, 64);
    switch_const<1, 2, 3, 4, 8>(nj <= 4 ? nj : 8, [&](auto s) {
      constexpr int NJ = decltype(s)::value;
      sage_max_fwd_kernel<NJ, sage_rows_in_flight(NJ)><<<(unsigned)ceil_div(num_nodes, 4), 256, 0, st>>>(
          num_nodes, in_rowptr, in_src, X, ldx, D, out, ldo, arg, lda, blk_amax, out_row_amax);
      return MVML_OK;
    });
  }
  if (int rc = check_launch("sage_max_fwd_kernel")) return rc;
  return launch_rows_amax(num_nodes, out_row_amax, out_amax, st);
}

extern "C" int mvml_sage_max_bwd(int64_t num_nodes, const int32_t* out_rowptr, const int32_t* out_dst,
                                 const int32_t* out_inslot, const float* G, int64_t ldg, const int32_t* arg,
                                 int64_t lda, int D, const float* P, int64_t ldp, float* gX, int64_t ldgx,
                                 void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "sage_max_bwd: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "sage_max_bwd: D must be a positive multiple of 4 <= 2048 (got %d)", D);
  MVML_REQUIRE(out_rowptr != nullptr && out_dst != nullptr && out_inslot != nullptr,
               "sage_max_bwd: out_rowptr, out_dst and out_inslot are required");
  MVML_REQUIRE(row_ok(G, ldg, D) && row_ok(arg, lda, D) && row_ok(gX, ldgx, D),
               "sage_max_bwd: G, arg and gX must be 16-byte aligned with row strides >= D that are multiples of 4");
  MVML_REQUIRE(P == nullptr || row_ok(P, ldp, D),
               "sage_max_bwd: P must be 16-byte aligned with a row stride ldp >= D that is a multiple of 4");
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(!rows_meet(G, ldg, gX, ldgx, num_nodes, D) && !rows_meet(arg, lda, gX, ldgx, num_nodes, D),
               "sage_max_bwd: gX must not alias G or arg");
  const hipStream_t st = as_stream(stream);
  if (D <= 64 && option(MVML_OPT_SAGE_SUBWAVE) != 0) {
    sage_max_bwd_sub_kernel<4><<<(unsigned)ceil_div(num_nodes, 16), 256, 0, st>>>(
        num_nodes, out_rowptr, out_dst, out_inslot, G, ldg, arg, lda, D, P, ldp, gX, ldgx);
  } else {
    const int nj = (int)ceil_div(D / 4, 64);
    switch_const<1, 2, 3, 4, 8>(nj <= 4 ? nj : 8, [&](auto s) {
      constexpr int NJ = decltype(s)::value;
      sage_max_bwd_kernel<NJ, sage_rows_in_flight(NJ)><<<(unsigned)ceil_div(num_nodes, 4), 256, 0, st>>>(
          num_nodes, out_rowptr, out_dst, out_inslot, G, ldg, arg, lda, D, P, ldp, gX, ldgx);
      return MVML_OK;
    });
  }
  return check_launch("sage_max_bwd_kernel");
}

extern "C" int mvml_sage_gcn_scale(int64_t num_nodes, const int32_t* in_rowptr, float* scale, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "sage_gcn_scale: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(in_rowptr != nullptr && scale != nullptr, "sage_gcn_scale: in_rowptr and scale are required");
  if (num_nodes == 0) return MVML_OK;
  sage_gcn_scale_kernel<<<(unsigned)ceil_div(num_nodes, 256), 256, 0, as_stream(stream)>>>(num_nodes, in_rowptr, scale);
  return check_launch("sage_gcn_scale_kernel");
}

extern "C" int mvml_sage_self_add(int64_t num_nodes, const float* X, int64_t ldx, int D, const float* scale,
                                  const float* bias, int act, float* out, int64_t ldo, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "sage_self_add: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "sage_self_add: D must be a positive multiple of 4 <= 2048 (got %d)", D);
  MVML_REQUIRE(act == 0 || act == 1, "sage_self_add: bad act %d", act);
  MVML_REQUIRE(scale != nullptr, "sage_self_add: scale is required");
  MVML_REQUIRE(row_ok(X, ldx, D) && row_ok(out, ldo, D),
               "sage_self_add: X and out must be 16-byte aligned with row strides ldx, ldo >= D that are multiples of 4");
  MVML_REQUIRE(aligned16(bias), "sage_self_add: bias must be 16-byte aligned");
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(!rows_meet(X, ldx, out, ldo, num_nodes, D), "sage_self_add: out must not alias X");
  sage_self_add_kernel<<<(unsigned)ceil_div(num_nodes * (D / 4), 256), 256, 0, as_stream(stream)>>>(
      num_nodes, X, ldx, D, scale, bias, act, out, ldo);
  return check_launch("sage_self_add_kernel");
}
