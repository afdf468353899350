// Per-molecule pooling of atom rows (dgl 0.9.1 SumPooling / AvgPooling / MaxPooling, the readouts
// of dgllife's GINPredictor; restated, parity with dgl unpinned) and its backward.
//
//   sum:   out[g] = sum_n X[n]                 n ascending over [node_offsets[g], node_offsets[g+1])
//   mean:  out[g] = (sum_n X[n]) / count       one division of the finished sum
//   max:   out[g] = max_n X[n],  argmax[g][c] = the lowest atom index that attains it
//
// One wave per molecule, as mvml_wsum_max_fwd (readout.hip): lanes on the float4 columns
// c = lane + 64 j with the last slot masked, the atoms walked in order with U rows in flight, every
// add an __fadd_rn from 0, so the bits of a molecule's row depend on nothing but its atoms' rows.
// The backward is one wave per molecule too: it loads the molecule's gradient row once and writes
// every gX row of the molecule once (sum: the row; mean: the row divided by the count; max: the
// row's elements where argmax names this atom, 0 elsewhere).  No atomics.
#include "gat_agg_common.h"

namespace mvml {
namespace {

constexpr int kPoolSum = 0, kPoolMean = 1, kPoolMax = 2;

typedef int mvml_i4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int4 ldi4(const int32_t* p) { return *reinterpret_cast<const int4*>(p); }
__device__ __forceinline__ void sti4(int32_t* p, int4 v) { *reinterpret_cast<int4*>(p) = v; }
__device__ __forceinline__ float4 add4_rn(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float4 div4_rn(float4 a, float d) {
  return make_float4(__fdiv_rn(a.x, d), __fdiv_rn(a.y, d), __fdiv_rn(a.z, d), __fdiv_rn(a.w, d));
}
// one element of the running maximum: the first atom always enters, later ones on >
__device__ __forceinline__ void max_step(float x, int n, bool first, float& m, int& a) {
  const bool up = first || x > m;
  m = up ? x : m;
  a = up ? n : a;
}

template <int NJ, int U>
__global__ void __launch_bounds__(256)
segment_pool_fwd_kernel(int64_t B, int64_t N, int D, int mode, const int64_t* __restrict__ node_offsets,
                        const float* __restrict__ X, int64_t ldx, float* __restrict__ out, int64_t ldo,
                        int32_t* __restrict__ argmax, int64_t lda) {
  const int lane = threadIdx.x & 63;
  const int64_t g = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (g >= B) return;
  bool ok[NJ];
  float4 acc[NJ];
  int4 am[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    ok[j] = 4 * (lane + 64 * j) < D;
    acc[j] = f4(0.f);  // a molecule without atoms: 0 and -1
    am[j] = make_int4(-1, -1, -1, -1);
  }
  // (offsets past the atom rows cannot come from mvml_build_csr: clamped all the same)
  const int64_t n0 = min(max(node_offsets[g], (int64_t)0), N), n1 = min(node_offsets[g + 1], N);
  for (int64_t nb = n0; nb < n1; nb += U) {
    float4 x[U][NJ];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t n = min(nb + u, n1 - 1);  // past the molecule: a duplicate row, not used
#pragma unroll
      for (int j = 0; j < NJ; ++j) x[u][j] = ok[j] ? ld4nt(X + n * ldx + 4 * (lane + 64 * j)) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (nb + u < n1) {  // (uniform)
        const int n = (int)(nb + u);
        const bool first = nb + u == n0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (mode == kPoolMax) {
            max_step(x[u][j].x, n, first, acc[j].x, am[j].x);
            max_step(x[u][j].y, n, first, acc[j].y, am[j].y);
            max_step(x[u][j].z, n, first, acc[j].z, am[j].z);
            max_step(x[u][j].w, n, first, acc[j].w, am[j].w);
          } else {
            acc[j] = add4_rn(acc[j], x[u][j]);
          }
        }
      }
    }
  }
  const float cnt = (float)(n1 - n0);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (!ok[j]) continue;
    const int c = 4 * (lane + 64 * j);
    float4 o = acc[j];
    if (mode == kPoolMean && n1 > n0) o = div4_rn(o, cnt);
    st4(out + g * ldo + c, o);
    if (mode == kPoolMax) sti4(argmax + g * lda + c, am[j]);
  }
}

template <int NJ>
__global__ void __launch_bounds__(256)
segment_pool_bwd_kernel(int64_t B, int64_t N, int D, int mode, const int64_t* __restrict__ node_offsets,
                        const float* __restrict__ G, int64_t ldg, const int32_t* __restrict__ argmax, int64_t lda,
                        float* __restrict__ gX, int64_t ldgx) {
  const int lane = threadIdx.x & 63;
  const int64_t g = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (g >= B) return;
  // (offsets past the atom rows cannot come from mvml_build_csr: clamped all the same)
  const int64_t n0 = min(max(node_offsets[g], (int64_t)0), N), n1 = min(node_offsets[g + 1], N);
  if (n1 <= n0) return;  // an empty molecule takes no gradient
  const float cnt = (float)(n1 - n0);
  bool ok[NJ];
  float4 gr[NJ];
  int4 am[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = 4 * (lane + 64 * j);
    ok[j] = c < D;
    gr[j] = ok[j] ? ld4(G + g * ldg + c) : f4(0.f);
    if (mode == kPoolMean) gr[j] = div4_rn(gr[j], cnt);
    am[j] = (ok[j] && mode == kPoolMax) ? ldi4(argmax + g * lda + c) : make_int4(-1, -1, -1, -1);
  }
  for (int64_t n = n0; n < n1; ++n) {
    const int a = (int)n;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (!ok[j]) continue;
      float4 o = gr[j];
      if (mode == kPoolMax)
        o = make_float4(am[j].x == a ? o.x : 0.f, am[j].y == a ? o.y : 0.f, am[j].z == a ? o.z : 0.f,
                        am[j].w == a ? o.w : 0.f);
      st4nt(gX + n * ldgx + 4 * (lane + 64 * j), o);
    }
  }
}

inline int check_pool(const char* who, int64_t B, int64_t N, int D, int mode) {
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "%s: D must be a positive multiple of 4 <= 2048 (got %d)", who, D);
  MVML_REQUIRE(mode >= kPoolSum && mode <= kPoolMax, "%s: mode must be 0 (sum), 1 (mean) or 2 (max), got %d", who, mode);
  MVML_REQUIRE(B >= 0 && N >= 0 && N < (int64_t(1) << 31), "%s: bad B / N (atom indices are int32)", who);
  return MVML_OK;
}

inline bool ranges_meet(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const char *a0 = (const char*)a, *b0 = (const char*)b;
  return !(a0 + abytes <= b0 || b0 + bbytes <= a0);
}
inline int64_t rows_bytes(int64_t n, int64_t ld, int D) { return 4 * ((n - 1) * ld + D); }

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_segment_pool_fwd(int64_t B, int64_t N, int D, int mode, const int64_t* node_offsets,
                                     const float* X, int64_t ldx, float* out, int64_t ldo, int32_t* argmax,
                                     int64_t lda, void* stream) {
  clear_error();
  if (int rc = check_pool("segment_pool_fwd", B, N, D, mode)) return rc;
  MVML_REQUIRE(row_ok(out, ldo, D) && (N == 0 || row_ok(X, ldx, D)),
               "segment_pool_fwd: X and out must be 16-byte aligned with row strides >= D that are multiples of 4");
  MVML_REQUIRE(mode != kPoolMax || row_ok(argmax, lda, D),
               "segment_pool_fwd: max needs argmax, 16-byte aligned with a row stride >= D that is a multiple of 4");
  if (B == 0) return MVML_OK;
  MVML_REQUIRE(node_offsets != nullptr, "segment_pool_fwd: node_offsets is required");
  MVML_REQUIRE(N == 0 || !ranges_meet(X, rows_bytes(N, ldx, D), out, rows_bytes(B, ldo, D)),
               "segment_pool_fwd: out must not alias X");
  const int nj = (int)ceil_div(D / 4, 64);
  switch_const<1, 2, 3, 4, 8>(nj <= 4 ? nj : 8, [&](auto s) {
    constexpr int NJ = decltype(s)::value;
    segment_pool_fwd_kernel<NJ, (NJ <= 2 ? 4 : 2)><<<(unsigned)ceil_div(B, 4), 256, 0, as_stream(stream)>>>(
        B, N, D, mode, node_offsets, X, ldx, out, ldo, argmax, lda);
    return MVML_OK;
  });
  return check_launch("segment_pool_fwd_kernel");
}

extern "C" int mvml_segment_pool_bwd(int64_t B, int64_t N, int D, int mode, const int64_t* node_offsets,
                                     const float* G, int64_t ldg, const int32_t* argmax, int64_t lda, float* gX,
                                     int64_t ldgx, void* stream) {
  clear_error();
  if (int rc = check_pool("segment_pool_bwd", B, N, D, mode)) return rc;
  if (B == 0 || N == 0) return MVML_OK;
  MVML_REQUIRE(row_ok(G, ldg, D) && row_ok(gX, ldgx, D),
               "segment_pool_bwd: G and gX must be 16-byte aligned with row strides >= D that are multiples of 4");
  MVML_REQUIRE(mode != kPoolMax || row_ok(argmax, lda, D),
               "segment_pool_bwd: max needs argmax, 16-byte aligned with a row stride >= D that is a multiple of 4");
  MVML_REQUIRE(node_offsets != nullptr, "segment_pool_bwd: node_offsets is required");
  MVML_REQUIRE(!ranges_meet(G, rows_bytes(B, ldg, D), gX, rows_bytes(N, ldgx, D)),
               "segment_pool_bwd: gX must not alias G");
  const int nj = (int)ceil_div(D / 4, 64);
  switch_const<1, 2, 3, 4, 8>(nj <= 4 ? nj : 8, [&](auto s) {
    constexpr int NJ = decltype(s)::value;
    segment_pool_bwd_kernel<NJ><<<(unsigned)ceil_div(B, 4), 256, 0, as_stream(stream)>>>(
        B, N, D, mode, node_offsets, G, ldg, argmax, lda, gX, ldgx);
    return MVML_OK;
  });
  return check_launch("segment_pool_bwd_kernel");
}
