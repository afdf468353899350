// Weighted-sum-and-max readout (dgllife 0.3.0 WeightedSumAndMax: WeightAndSum's sigmoid gate
// over sum_nodes, next to max_nodes): per molecule g with atoms n in [off[g], off[g+1])
//   s_n = sigmoid(<W, x_n> + b);  out[g] = [ sum_n s_n x_n | max_n x_n ].
// Same shape as the Set2Set segment pass (set2set.hip): one wavefront per molecule streams its
// atoms' rows once, a lane holding float4 column groups 4*(lane + 64*c), c < NV = ceil(D / 256).
// Where that pass keeps one row in flight per wave, these load 2 or 4 rows (RowsAhead) and run
// their reduction chains (dot -> wave_sum -> sigmoid) side by side before the in-order
// accumulation, so a 400-atom molecule is not 400 dependent load -> reduce steps.
// Atoms are accumulated in index order and nothing is added atomically: the outputs are a fixed
// function of the inputs, bitwise equal run to run.
#include "common.h"
#include "wave_ops.h"

namespace mvml {
namespace {

// sigmoid on v_exp_f32 and v_rcp_f32 (1 ulp each; the exponent's x * log2(e) rounding adds
// |x| * 2^-24 relative, 3e-6 at the |x| = 50 where the gate has saturated): a quarter of the
// instructions of expf and an IEEE division, in a loop whose time followed its vector
// instruction count where it followed nothing else ("Weighted-sum-and-max")
__device__ __forceinline__ float sigm(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

// Rows in flight per wave (the row buffer is 4 NV VGPRs per row).  The backward holds five
// vectors per column slot where the forward holds four, and takes fewer rows for the occupancy.
template <int NV>
struct RowsAhead {
  static constexpr int fwd = NV <= 2 ? 4 : 2;
  static constexpr int bwd = NV <= 1 ? 4 : 2;
};

// The molecule of this wave, as a wave-uniform (scalar) value: the offsets, the atom loop and the
// per-atom gate addresses then live in SGPRs.
__device__ __forceinline__ int64_t wave_molecule() {
  return (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// max with the lowest index on ties: a strict > walking the atoms in order (NaN never wins)
__device__ __forceinline__ void take_max(float x, int n, float& m, int& am) {
  if (x > m) {
    m = x;
    am = n;
  }
}

template <int NV>
__global__ void __launch_bounds__(256)
wsum_max_fwd_kernel(int64_t B, int D, const int64_t* __restrict__ node_off, const float* __restrict__ X,
                    int64_t ldx, const float* __restrict__ W, const float* __restrict__ bias,
                    float* __restrict__ out, int64_t ldo, float* __restrict__ gate,
                    int32_t* __restrict__ argmax, int64_t lda) {
  constexpr int U = RowsAhead<NV>::fwd;
  const int lane = threadIdx.x & 63;
  const int64_t g = wave_molecule();
  if (g >= B) return;
  const int64_t n0 = node_off[g], n1 = node_off[g + 1];
  const float b = bias[0];
  float4 w[NV], acc[NV], mx[NV];
  int4 am[NV];
  bool ok[NV];
  int lcol[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int col = 4 * (lane + 64 * c);
    ok[c] = col < D;
    // a lane past the row's end reads the row's last column group instead (no select and no
    // branch per load in the loop): its gate weight is 0 and nothing of it is stored
    lcol[c] = min(col, D - 4);
    w[c] = ok[c] ? ld4(W + col) : make_float4(0, 0, 0, 0);
    acc[c] = make_float4(0, 0, 0, 0);
    mx[c] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    am[c] = make_int4(-1, -1, -1, -1);
  }
  for (int64_t base = n0; base < n1; base += U) {
    float4 x[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // past the molecule's end: its last row again (in bounds, not used)
      const int64_t n = min<int64_t>(base + u, n1 - 1);
#pragma unroll
      for (int c = 0; c < NV; ++c) x[u][c] = ld4(X + n * ldx + lcol[c]);
    }
    // the U gates first, with no branch between them: U independent dot -> wave_sum -> sigmoid
    // chains the scheduler can interleave (a row past the end repeats the last one, unused)
    float sg[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float part = 0.f;
#pragma unroll
      for (int c = 0; c < NV; ++c) part += dot4_contract(x[u][c], w[c]);
      sg[u] = sigm(wave_sum(part) + b);
    }
    // one gate store per batch: lane u writes row u's
    float gv = sg[0];
#pragma unroll
    for (int u = 1; u < U; ++u) gv = lane == u ? sg[u] : gv;
    if (lane < U && base + lane < n1) gate[base + lane] = gv;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t n = base + u;
      if (n >= n1) break;  // uniform
      const float s = sg[u];
      const int ni = (int)n;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        acc[c].x += s * x[u][c].x;
        acc[c].y += s * x[u][c].y;
        acc[c].z += s * x[u][c].z;
        acc[c].w += s * x[u][c].w;
        take_max(x[u][c].x, ni, mx[c].x, am[c].x);
        take_max(x[u][c].y, ni, mx[c].y, am[c].y);
        take_max(x[u][c].z, ni, mx[c].z, am[c].z);
        take_max(x[u][c].w, ni, mx[c].w, am[c].w);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NV; ++c)
    if (ok[c]) {
      const int col = 4 * (lane + 64 * c);
      st4(out + g * ldo + col, acc[c]);
      // a column no atom owns (a molecule without atoms): max 0, argmax -1
      st4(out + g * ldo + D + col,
          make_float4(am[c].x < 0 ? 0.f : mx[c].x, am[c].y < 0 ? 0.f : mx[c].y,
                      am[c].z < 0 ? 0.f : mx[c].z, am[c].w < 0 ? 0.f : mx[c].w));
      *reinterpret_cast<int4*>(argmax + g * lda + col) = am[c];
    }
}

// Backward, the same molecule wave: t_n = <g_s, x_n>, c_n = s_n (1 - s_n) t_n,
//   gX[n] = s_n g_s + c_n W + [argmax == n] g_m,   partial: sum_n c_n x_n | sum_n c_n.
// The four molecules of a workgroup add their partials through LDS in wave order 0..3 into row
// blockIdx.x of part ([gridDim.x][ldp]: columns [0, D) the weight term, column D the bias term);
// the column sums of part are dL/dW and dL/db.
template <int NV>
__global__ void __launch_bounds__(256)
wsum_max_bwd_kernel(int64_t B, int D, const int64_t* __restrict__ node_off, const float* __restrict__ X,
                    int64_t ldx, const float* __restrict__ W, const float* __restrict__ gate,
                    const int32_t* __restrict__ argmax, int64_t lda, const float* __restrict__ g_out,
                    int64_t ldgo, float* __restrict__ gX, int64_t ldgx, float* __restrict__ part,
                    int64_t ldp) {
  constexpr int U = RowsAhead<NV>::bwd;
  __shared__ float4 red[4][NV * 64];
  __shared__ float redb[4];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t g = wave_molecule();
  // a wave past the last molecule walks no atoms and adds a zero partial (it still meets the
  // barrier below)
  const bool live = g < B;
  const int64_t n0 = live ? node_off[g] : 0, n1 = live ? node_off[g + 1] : 0;
  float4 w[NV], gs[NV], gm[NV], pw[NV];
  int4 am[NV];
  bool ok[NV];
  int lcol[NV];
  float pb = 0.f;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int col = 4 * (lane + 64 * c);
    ok[c] = col < D;
    lcol[c] = min(col, D - 4);  // as in the forward: g_s is 0 there and nothing of it is stored
    const bool ld = ok[c] && n1 > n0;
    w[c] = ld ? ld4(W + col) : make_float4(0, 0, 0, 0);
    gs[c] = ld ? ld4(g_out + g * ldgo + col) : make_float4(0, 0, 0, 0);
    gm[c] = ld ? ld4(g_out + g * ldgo + D + col) : make_float4(0, 0, 0, 0);
    am[c] = ld ? *reinterpret_cast<const int4*>(argmax + g * lda + col) : make_int4(-1, -1, -1, -1);
    pw[c] = make_float4(0, 0, 0, 0);
  }
  for (int64_t base = n0; base < n1; base += U) {
    float4 x[U][NV];
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t n = min<int64_t>(base + u, n1 - 1);
      s[u] = gate[n];
#pragma unroll
      for (int c = 0; c < NV; ++c) x[u][c] = ld4(X + n * ldx + lcol[c]);
    }
    float t[U];  // the U dot -> wave_sum chains first, independent of one another
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float part_t = 0.f;
#pragma unroll
      for (int c = 0; c < NV; ++c) part_t += dot4_contract(x[u][c], gs[c]);
      t[u] = wave_sum(part_t);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t n = base + u;
      if (n >= n1) break;  // uniform
      const float sn = s[u];
      const float cn = sn * (1.f - sn) * t[u];
      pb += cn;
      const int ni = (int)n;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        pw[c].x += cn * x[u][c].x;
        pw[c].y += cn * x[u][c].y;
        pw[c].z += cn * x[u][c].z;
        pw[c].w += cn * x[u][c].w;
        if (ok[c]) {
          float4 r;
          r.x = sn * gs[c].x + cn * w[c].x + (am[c].x == ni ? gm[c].x : 0.f);
          r.y = sn * gs[c].y + cn * w[c].y + (am[c].y == ni ? gm[c].y : 0.f);
          r.z = sn * gs[c].z + cn * w[c].z + (am[c].z == ni ? gm[c].z : 0.f);
          r.w = sn * gs[c].w + cn * w[c].w + (am[c].w == ni ? gm[c].w : 0.f);
          st4(gX + n * ldgx + 4 * (lane + 64 * c), r);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NV; ++c) red[wv][lane + 64 * c] = pw[c];
  if (lane == 0) redb[wv] = pb;  // every lane holds the same sum
  __syncthreads();
  float* prow = part + (int64_t)blockIdx.x * ldp;
  for (int i = threadIdx.x; i < NV * 64; i += 256) {
    if (4 * i >= D) break;
    const float4 a = red[0][i], b4 = red[1][i], c4 = red[2][i], d4 = red[3][i];
    st4(prow + 4 * i, make_float4(((a.x + b4.x) + c4.x) + d4.x, ((a.y + b4.y) + c4.y) + d4.y,
                                  ((a.z + b4.z) + c4.z) + d4.z, ((a.w + b4.w) + c4.w) + d4.w));
  }
  if (threadIdx.x == 0) prow[D] = ((redb[0] + redb[1]) + redb[2]) + redb[3];
}

int check_d(int D, const char* who) {
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024, "%s: feature size must be a multiple of 4 <= 1024 (got %d)", who, D);
  return MVML_OK;
}

}  // namespace
}  // namespace mvml

using namespace mvml;

#define MVML_NV_SWITCH(KERNEL, GRID, ...)                                                   \
  switch ((int)ceil_div(D, 256)) {                                                          \
    case 1: KERNEL<1><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;                            \
    case 2: KERNEL<2><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;                            \
    case 3: KERNEL<3><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;                            \
    default: KERNEL<4><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;                           \
  }

extern "C" int mvml_wsum_max_fwd(int64_t B, int64_t N, int D, const int64_t* node_offsets,
                                 const float* X, int64_t ldx, const float* W, const float* bias,
                                 float* out, int64_t ldo, float* gate, int32_t* argmax, int64_t lda,
                                 void* stream) {
  clear_error();
  int rc = check_d(D, "wsum_max_fwd");
  if (rc) return rc;
  MVML_REQUIRE(B >= 0 && N >= 0 && N <= INT32_MAX, "wsum_max_fwd: bad B / N (atom indices are int32)");
  MVML_REQUIRE(ldx >= D && ldx % 4 == 0 && ldo >= 2 * D && ldo % 4 == 0 && lda >= D && lda % 4 == 0,
               "wsum_max_fwd: row pitches must be multiples of 4 with ldx >= D, ldo >= 2 D, lda >= D");
  if (B == 0 || N == 0) return MVML_OK;
  MVML_REQUIRE(node_offsets && X && W && bias && out && gate && argmax, "wsum_max_fwd: null pointer");
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)ceil_div(B, 4);
  MVML_NV_SWITCH(wsum_max_fwd_kernel, grid, B, D, node_offsets, X, ldx, W, bias, out, ldo, gate,
                 argmax, lda)
  return check_launch("wsum_max_fwd_kernel");
}

extern "C" int64_t mvml_wsum_max_bwd_part_rows(int64_t B) { return B > 0 ? ceil_div(B, 4) : 0; }

extern "C" int mvml_wsum_max_bwd(int64_t B, int64_t N, int D, const int64_t* node_offsets,
                                 const float* X, int64_t ldx, const float* W, const float* gate,
                                 const int32_t* argmax, int64_t lda, const float* g_out,
                                 int64_t ldgo, float* gX, int64_t ldgx, float* part, int64_t ldp,
                                 void* stream) {
  clear_error();
  int rc = check_d(D, "wsum_max_bwd");
  if (rc) return rc;
  MVML_REQUIRE(B >= 0 && N >= 0 && N <= INT32_MAX, "wsum_max_bwd: bad B / N (atom indices are int32)");
  MVML_REQUIRE(ldx >= D && ldx % 4 == 0 && ldgo >= 2 * D && ldgo % 4 == 0 && lda >= D && lda % 4 == 0 &&
                   ldgx >= D && ldgx % 4 == 0 && ldp >= D + 4 && ldp % 4 == 0,
               "wsum_max_bwd: row pitches must be multiples of 4 with ldx, lda, ldgx >= D, ldgo >= 2 D, "
               "ldp >= D + 4");
  if (B == 0 || N == 0) return MVML_OK;
  MVML_REQUIRE(node_offsets && X && W && gate && argmax && g_out && gX && part, "wsum_max_bwd: null pointer");
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)ceil_div(B, 4);
  MVML_NV_SWITCH(wsum_max_bwd_kernel, grid, B, D, node_offsets, X, ldx, W, gate, argmax, lda, g_out,
                 ldgo, gX, ldgx, part, ldp)
  return check_launch("wsum_max_bwd_kernel");
}
