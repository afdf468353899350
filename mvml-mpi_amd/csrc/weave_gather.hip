// Weave's Gaussian-histogram readout (dgllife 0.3.0 WeaveGather, Kearnes et al. "Molecular graph
// convolutions"; restated, parity with dgllife unpinned) without the [N, F K] expansion in memory.
// For an atom value x = X[n][f] and the K memberships (mu_k, sigma_k):
//
//   q_k = exp(-(x - mu_k)^2 / (2 sigma_k^2)) + 1e-7     p_k = q_k / sum_j q_j
//   out[g][f K + k] = sum over the atoms n of molecule g, ascending, of p_k(X[n][f])
//
// weave_gather_fwd_kernel: one wave owns one molecule and 64 consecutive columns f, lane = column, so
// an atom row is one coalesced 256-B read per wave and the K memberships of a value, their sum and the
// K running sums all stay in the lane's registers (K is a template argument: no array is indexed at
// run time).  The memberships arrive by value in the kernel arguments, as mu_k and 1 / (2 sigma_k^2),
// and are wave-uniform.  U atom rows are in flight.  Every add is an __fadd_rn from 0 in atom order, so a
// molecule's bits depend on nothing but its atoms' rows.  The lane's K sums are K consecutive floats of
// the output row and the wave's 64 K floats one contiguous run: they go through a wave-private LDS
// window ([column][k], as they lie in memory) and leave as K coalesced stores.
//
// weave_gather_bwd_kernel: the same split.  The molecule's gradient run dG[g][f0 K ..] comes in through
// the window, K values per lane, once; then one pass over the atom rows recomputes e_k = q_k - 1e-7 and
// S = sum_j q_j and writes
//   dX[n][f] = (1 / S) sum_k dq_k (dG_k - c),   dq_k = -(x - mu_k) / sigma_k^2 * e_k,   c = sum_k dG_k p_k
// which is sum_k dG_k (dq_k - p_k sum_j dq_j) / S with the common term taken out before the products.
//
// tanh_fwd_kernel / tanh_bwd_kernel: the readout's activation element-wise, the derivative 1 - y^2 from
// the output.  No atomics anywhere: bitwise repeatable.
#include "wave_ops.h"

#include <cmath>

namespace mvml {
namespace {

constexpr int kWgMaxK = 16;    // memberships
constexpr int kWgMaxF = 1024;  // columns
constexpr int kWgCols = 64;    // columns per wave
constexpr float kWgFloor = 1e-7f;

struct WgArgs {
  int64_t B, N;
  int F, chunks;  // chunks = ceil(F / 64)
  const int64_t* node_offsets;
  const float* X;  // [N][ldx]
  int64_t ldx;
  const float* G;  // backward: dL/dout [B][ldg]
  int64_t ldg;
  float* out;  // forward: [B][ldo]; backward: dL/dX [N][ldo]
  int64_t ldo;
  float mu[kWgMaxK], h[kWgMaxK];  // h_k = 1 / (2 sigma_k^2)
};

// The wave's molecule, first column and atom range; false: nothing to do.
__device__ __forceinline__ bool wg_tile(const WgArgs& a, int64_t& g, int& f0, int64_t& n0, int64_t& n1) {
  const int64_t w = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= a.B * a.chunks) return false;
  g = w / a.chunks;
  f0 = (int)(w - g * a.chunks) * kWgCols;
  // (offsets past the atom rows cannot come from mvml_build_csr: clamped all the same)
  n0 = min(max(a.node_offsets[g], (int64_t)0), a.N);
  n1 = min(a.node_offsets[g + 1], a.N);
  return true;
}

// e_k = exp(-(x - mu_k)^2 h_k) and S = sum_k (e_k + 1e-7), k ascending
template <int K>
__device__ __forceinline__ float wg_members(const WgArgs& a, float x, float (&e)[K]) {
  float S = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float t = x - a.mu[k];
    e[k] = expf(-__fmul_rn(__fmul_rn(t, t), a.h[k]));
    S = __fadd_rn(S, __fadd_rn(e[k], kWgFloor));
  }
  return S;
}

template <int K, int U>
__global__ void __launch_bounds__(256) weave_gather_fwd_kernel(WgArgs a) {
  __shared__ float win[4][kWgCols * K];
  const int lane = threadIdx.x & 63;
  int64_t g, n0, n1;
  int f0;
  if (!wg_tile(a, g, f0, n0, n1)) return;  // (no workgroup barrier below: a wave may leave alone)
  const bool ok = f0 + lane < a.F;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;  // a molecule without atoms: zeros
  for (int64_t nb = n0; nb < n1; nb += U) {
    float x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t n = min(nb + u, n1 - 1);  // past the molecule: a duplicate row, not used
      x[u] = ok ? a.X[n * a.ldx + f0 + lane] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (nb + u < n1) {  // (uniform)
        float e[K];
        const float inv = __fdiv_rn(1.f, wg_members<K>(a, x[u], e));
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(__fadd_rn(e[k], kWgFloor), inv));
      }
    }
  }
  float* w = win[threadIdx.x >> 6];
#pragma unroll
  for (int k = 0; k < K; ++k) w[lane * K + k] = acc[k];
  wave_sync_wavefront_scope();
  const int cnt = min(kWgCols, a.F - f0) * K;  // the live columns' run; dead lanes' sums stay in LDS
  float* o = a.out + g * a.ldo + (int64_t)f0 * K;
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (lane + 64 * j < cnt) o[lane + 64 * j] = w[lane + 64 * j];
}

template <int K, int U>
__global__ void __launch_bounds__(256) weave_gather_bwd_kernel(WgArgs a) {
  __shared__ float win[4][kWgCols * K];
  const int lane = threadIdx.x & 63;
  int64_t g, n0, n1;
  int f0;
  if (!wg_tile(a, g, f0, n0, n1) || n1 <= n0) return;  // an empty molecule takes no gradient
  const bool ok = f0 + lane < a.F;
  float* w = win[threadIdx.x >> 6];
  const int cnt = min(kWgCols, a.F - f0) * K;
  const float* gr = a.G + g * a.ldg + (int64_t)f0 * K;
#pragma unroll
  for (int j = 0; j < K; ++j) w[lane + 64 * j] = lane + 64 * j < cnt ? gr[lane + 64 * j] : 0.f;
  wave_sync_wavefront_scope();
  float dg[K];
#pragma unroll
  for (int k = 0; k < K; ++k) dg[k] = w[lane * K + k];
  for (int64_t nb = n0; nb < n1; nb += U) {
    float x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t n = min(nb + u, n1 - 1);
      x[u] = ok ? a.X[n * a.ldx + f0 + lane] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (nb + u < n1) {  // (uniform)
        float e[K];
        const float inv = __fdiv_rn(1.f, wg_members<K>(a, x[u], e));
        float c = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) c = __fmaf_rn(dg[k], __fadd_rn(e[k], kWgFloor), c);
        c = __fmul_rn(c, inv);  // sum_k dG_k p_k
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float dq = __fmul_rn(__fmul_rn(a.mu[k] - x[u], 2.f * a.h[k]), e[k]);  // -(x - mu) / sigma^2 e
          d = __fmaf_rn(dq, dg[k] - c, d);
        }
        if (ok) a.out[(nb + u) * a.ldo + f0 + lane] = __fmul_rn(d, inv);
      }
    }
  }
}

__global__ void __launch_bounds__(256) tanh_fwd_kernel(int64_t n, const float* x, float* y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = tanhf(x[i]);
}
__global__ void __launch_bounds__(256) tanh_bwd_kernel(int64_t n, const float* y, const float* gy, float* gx) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    gx[i] = __fmul_rn(gy[i], __fmaf_rn(-y[i], y[i], 1.f));
}

// The shapes and memberships every entry point takes; fills a.mu, a.h, a.chunks.
int check_gather(const char* who, int64_t B, int64_t N, int F, int K, const float* means, const float* stds, WgArgs& a) {
  MVML_REQUIRE(F >= 4 && F % 4 == 0 && F <= kWgMaxF, "%s: F must be a multiple of 4 in [4, %d] (got %d)", who, kWgMaxF, F);
  MVML_REQUIRE(K >= 1 && K <= kWgMaxK, "%s: 1 to %d Gaussian memberships K (got %d)", who, kWgMaxK, K);
  MVML_REQUIRE(B >= 0 && B < (int64_t(1) << 28) && N >= 0 && N < (int64_t(1) << 31), "%s: bad B / N (%lld, %lld)", who,
               (long long)B, (long long)N);
  MVML_REQUIRE(means != nullptr && stds != nullptr, "%s: means and stds (host arrays of K floats) are required", who);
  for (int k = 0; k < K; ++k) {
    const float h = (float)(0.5 / ((double)stds[k] * (double)stds[k]));
    MVML_REQUIRE(std::isfinite(means[k]) && stds[k] > 0.f && std::isfinite(2.f * h) && h > 0.f,
                 "%s: membership %d needs a finite mean and a std > 0 whose 1 / std^2 is a finite float (got %g, %g)",
                 who, k, (double)means[k], (double)stds[k]);
    a.mu[k] = means[k];
    a.h[k] = h;
  }
  a.chunks = (int)ceil_div(F, kWgCols);
  return MVML_OK;
}

template <typename Fn>
int by_k(int K, Fn&& fn) {
  return switch_const<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(K, fn);
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_weave_gather_fwd(int64_t B, int64_t N, int F, int K, const float* means, const float* stds,
                                     const int64_t* node_offsets, const float* X, int64_t ldx, float* out, int64_t ldo,
                                     void* stream) {
  clear_error();
  WgArgs a{};
  if (int rc = check_gather("weave_gather_fwd", B, N, F, K, means, stds, a)) return rc;
  if (B == 0) return MVML_OK;
  MVML_REQUIRE(node_offsets != nullptr && row_ok(out, ldo, (int64_t)F * K) && (N == 0 || row_ok(X, ldx, F)),
               "weave_gather_fwd: node_offsets is required; X and out must be 16-byte aligned with row pitches that are "
               "multiples of 4 and >= F and F K");
  a.B = B, a.N = N, a.F = F, a.node_offsets = node_offsets, a.X = X, a.ldx = ldx, a.out = out, a.ldo = ldo;
  const unsigned grid = (unsigned)ceil_div(B * a.chunks, 4);
  by_k(K, [&](auto k) {
    weave_gather_fwd_kernel<decltype(k)::value, 4><<<grid, 256, 0, as_stream(stream)>>>(a);
    return MVML_OK;
  });
  return check_launch("weave_gather_fwd_kernel");
}

extern "C" int mvml_weave_gather_bwd(int64_t B, int64_t N, int F, int K, const float* means, const float* stds,
                                     const int64_t* node_offsets, const float* X, int64_t ldx, const float* G, int64_t ldg,
                                     float* gX, int64_t ldgx, void* stream) {
  clear_error();
  WgArgs a{};
  if (int rc = check_gather("weave_gather_bwd", B, N, F, K, means, stds, a)) return rc;
  if (B == 0 || N == 0) return MVML_OK;
  MVML_REQUIRE(node_offsets != nullptr && row_ok(G, ldg, (int64_t)F * K) && row_ok(X, ldx, F) && row_ok(gX, ldgx, F),
               "weave_gather_bwd: node_offsets is required; X, G and gX must be 16-byte aligned with row pitches that are "
               "multiples of 4 and >= F, F K and F");
  a.B = B, a.N = N, a.F = F, a.node_offsets = node_offsets, a.X = X, a.ldx = ldx, a.G = G, a.ldg = ldg, a.out = gX,
  a.ldo = ldgx;
  const unsigned grid = (unsigned)ceil_div(B * a.chunks, 4);
  by_k(K, [&](auto k) {
    weave_gather_bwd_kernel<decltype(k)::value, 4><<<grid, 256, 0, as_stream(stream)>>>(a);
    return MVML_OK;
  });
  return check_launch("weave_gather_bwd_kernel");
}

extern "C" int mvml_tanh_fwd(int64_t n, const float* x, float* y, void* stream) {
  clear_error();
  MVML_REQUIRE(n >= 0, "tanh_fwd: negative n");
  if (n == 0) return MVML_OK;
  MVML_REQUIRE(x != nullptr && y != nullptr, "tanh_fwd: x and y are required");
  tanh_fwd_kernel<<<(unsigned)std::min<int64_t>(ceil_div(n, 256), 8192), 256, 0, as_stream(stream)>>>(n, x, y);
  return check_launch("tanh_fwd_kernel");
}

extern "C" int mvml_tanh_bwd(int64_t n, const float* y, const float* g_y, float* g_x, void* stream) {
  clear_error();
  MVML_REQUIRE(n >= 0, "tanh_bwd: negative n");
  if (n == 0) return MVML_OK;
  MVML_REQUIRE(y != nullptr && g_y != nullptr && g_x != nullptr, "tanh_bwd: y, g_y and g_x are required");
  tanh_bwd_kernel<<<(unsigned)std::min<int64_t>(ceil_div(n, 256), 8192), 256, 0, as_stream(stream)>>>(n, y, g_y, g_x);
  return check_launch("tanh_bwd_kernel");
}
