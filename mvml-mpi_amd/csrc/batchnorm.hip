// torch.nn.BatchNorm1d(C) on a 2-D input [M, C] (affine, running statistics, numeric momentum),
// forward and backward, training and eval mode: the normalisation inside dgllife 0.3.0's
// MLPPredictor (GATPredictor / GATv2Predictor), and usable on atom rows between graph layers.
//
// Parallel over rows as well as columns (GraphNorm's one thread per (group, column) would walk a
// whole-batch group of 65,536 rows serially).  A workgroup of 256 threads is CT column lanes x RT
// rows in flight (CT = the power of two >= the row's float4 / float count, at most 64; RT =
// 256 / CT), so a wave reads whole coalesced row segments.  The M rows are cut into
// R = mvml_batchnorm1d_part_rows(M) stripes, one workgroup per (column tile, stripe):
//   pass 1  per-stripe column sums into the caller's workspace, part[2][R][C] (fp64), each thread
//           walking its rows in order, then a fixed tree over the RT row lanes in LDS;
//   reduce  the R partials of a column summed in a fixed order (16 lanes x 4 accumulators, then
//           a tree), and the statistics / parameter gradients finalised by one thread per column;
//   pass 2  the per-element normalisation (forward) or g_x (training backward).
// No float atomics: every result is bitwise repeatable, and a column's results do not depend on
// which column it is.
//
// Arithmetic is fp64 throughout (inputs / outputs fp32), as norm.hip's GraphNorm: x - mean
// cancels.  The variance comes from sums shifted by the column's FIRST ROW, k = x[0][c]:
//   S = sum (x - k),  Q = sum (x - k)^2,  mean = k + S / M,  var = Q / M - (S / M)^2
// so stripes add without a Chan combine.  The shift is itself a sample, hence
// var >= (k - mean)^2 / M = (S / M)^2 / M: the subtraction cancels at most a factor M + 1, and
// the relative error of var stays below ~M 2^-52 times the summation's growth — 1e-9 at two
// million rows, against the 1e-5 bar (tests/test_gpu_batchnorm.py: x + 1000, a constant column).
// x - k is exact in fp64 for fp32 inputs within 2^29 of each other in exponent.
#include "common.h"

namespace mvml {
namespace {

constexpr int kBnThreads = 256;
constexpr int kBnStripeRows = 64;    // rows per stripe until the stripe cap is reached
constexpr int kBnMaxStripes = 1024;  // 2 x 1024 x C doubles of partials at most

inline int64_t bn_part_rows(int64_t M) {
  return M < 1 ? 0 : std::min<int64_t>(ceil_div(M, kBnStripeRows), kBnMaxStripes);
}

// log2 of the column lanes of a workgroup for rows of cv vector elements
inline int bn_ct_log2(int64_t cv) {
  int l = 0;
  while (l < 6 && (int64_t(1) << l) < cv) ++l;
  return l;
}

template <int V>
__device__ __forceinline__ void bn_load(const float* p, double (&v)[V]) {
  if constexpr (V == 4) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
  } else {
    v[0] = p[0];
  }
}

template <int V>
__device__ __forceinline__ void bn_store(float* p, const double (&v)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  } else {
    p[0] = (float)v[0];
  }
}

// Sum of every value over the RT row lanes that share a column lane (fixed tree); the result is
// valid in the threads of row lane 0.
template <int NV>
__device__ __forceinline__ void bn_row_lane_sum(double (&v)[NV], int ctl) {
  __shared__ double red[NV][kBnThreads];
  const int t = threadIdx.x, ry = t >> ctl;
#pragma unroll
  for (int i = 0; i < NV; ++i) red[i][t] = v[i];
  __syncthreads();
  for (int h = (kBnThreads >> ctl) >> 1; h > 0; h >>= 1) {
    if (ry < h) {
#pragma unroll
      for (int i = 0; i < NV; ++i) red[i][t] += red[i][t + (h << ctl)];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = red[i][t];
}

// pass 1 of the training forward: part[0][s][c] = sum (x - k), part[1][s][c] = sum (x - k)^2 over
// stripe s = blockIdx.y (rows [s rs, min(M, (s + 1) rs)); an empty stripe writes zeros)
template <int V>
__global__ void __launch_bounds__(kBnThreads) bn_fwd_stats_kernel(int64_t M, int C, int ctl, int64_t rs,
                                                                   const float* __restrict__ x, int64_t ldx,
                                                                   double* __restrict__ part, int64_t R) {
  const int rt = kBnThreads >> ctl;
  const int cx = threadIdx.x & ((1 << ctl) - 1), ry = threadIdx.x >> ctl;
  const int64_t c0 = (((int64_t)blockIdx.x << ctl) + cx) * V;
  const bool live = c0 < C;
  const int64_t s = blockIdx.y;
  const int64_t r0 = s * rs, r1 = std::min<int64_t>(M, r0 + rs);
  double acc[2 * V];
#pragma unroll
  for (int j = 0; j < 2 * V; ++j) acc[j] = 0.0;
  if (live) {
    double k[V];
    bn_load<V>(x + c0, k);
    int64_t r = r0 + ry;
    for (; r + 3 * rt < r1; r += 4 * rt) {  // four rows in flight
      double v[4][V];
#pragma unroll
      for (int u = 0; u < 4; ++u) bn_load<V>(x + (r + u * rt) * ldx + c0, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const double d = v[u][j] - k[j];
          acc[j] += d;
          acc[V + j] = fma(d, d, acc[V + j]);
        }
      }
    }
    for (; r < r1; r += rt) {
      double v[V];
      bn_load<V>(x + r * ldx + c0, v);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double d = v[j] - k[j];
        acc[j] += d;
        acc[V + j] = fma(d, d, acc[V + j]);
      }
    }
  }
  bn_row_lane_sum<2 * V>(acc, ctl);
  if (live && ry == 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      part[(0 * R + s) * C + c0 + j] = acc[j];
      part[(1 * R + s) * C + c0 + j] = acc[V + j];
    }
  }
}

// The R stripe partials of both sums of 16 columns, in a fixed order: 16 stripe lanes per column
// (s = lane, lane + 16, ...; four accumulators keep the loads in flight), then a tree in LDS.
// Valid in the threads of stripe lane 0.
__device__ __forceinline__ void bn_sum_stripes(int C, int64_t R, const double* __restrict__ part, int col,
                                               double& o0, double& o1) {
  const int c = threadIdx.x & 15, lane = threadIdx.x >> 4;
  double a[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  if (col < C) {
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const double* p = part + (int64_t)w * R * C + col;
      int64_t s = lane;
      for (; s + 48 < R; s += 64) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[w][u] += p[(s + 16 * u) * C];
      }
      for (; s < R; s += 16) a[w][0] += p[s * C];
    }
  }
  __shared__ double red[2][16][17];
  red[0][lane][c] = (a[0][0] + a[0][1]) + (a[0][2] + a[0][3]);
  red[1][lane][c] = (a[1][0] + a[1][1]) + (a[1][2] + a[1][3]);
  __syncthreads();
  for (int h = 8; h > 0; h >>= 1) {
    if (lane < h) {
      red[0][lane][c] += red[0][lane + h][c];
      red[1][lane][c] += red[1][lane + h][c];
    }
    __syncthreads();
  }
  o0 = red[0][0][c];
  o1 = red[1][0][c];
}

// Batch statistics of 16 columns from the stripe partials, the running-statistics update and the
// batch counter (torch's: momentum on the biased mean, on the UNBIASED variance).
__global__ void __launch_bounds__(kBnThreads) bn_fwd_finalize_kernel(
    int64_t M, int C, int64_t R, const double* __restrict__ part, const float* __restrict__ x, double momentum,
    double eps, float* __restrict__ running_mean, float* __restrict__ running_var,
    int64_t* __restrict__ num_batches_tracked, double* __restrict__ save_mean, double* __restrict__ save_invstd) {
  const int col = blockIdx.x * 16 + (threadIdx.x & 15);
  double S, Q;
  bn_sum_stripes(C, R, part, col, S, Q);
  if (blockIdx.x == 0 && threadIdx.x == 0 && num_batches_tracked) num_batches_tracked[0] += 1;
  if ((threadIdx.x >> 4) != 0 || col >= C) return;
  const double n = (double)M;
  const double sm = S / n;
  const double mean = (double)x[col] + sm;
  const double var = fmax(Q / n - sm * sm, 0.0);
  save_mean[col] = mean;
  save_invstd[col] = 1.0 / sqrt(var + eps);
  if (running_mean) running_mean[col] = (float)((1.0 - momentum) * (double)running_mean[col] + momentum * mean);
  if (running_var)
    running_var[col] = (float)((1.0 - momentum) * (double)running_var[col] + momentum * (var * n / (n - 1.0)));
}

// eval mode: the statistics are the running ones
__global__ void bn_eval_stats_kernel(int C, const float* __restrict__ running_mean,
                                     const float* __restrict__ running_var, double eps,
                                     double* __restrict__ save_mean, double* __restrict__ save_invstd) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= C) return;
  save_mean[col] = (double)running_mean[col];
  save_invstd[col] = 1.0 / sqrt((double)running_var[col] + eps);
}

// pass 2 of the forward: y = (x - mean) invstd weight + bias, every element on its own (a row's
// output depends on that row and the statistics only)
template <int V>
__global__ void __launch_bounds__(kBnThreads) bn_fwd_apply_kernel(int64_t M, int C, int ctl,
                                                                   const float* __restrict__ x, int64_t ldx,
                                                                   const float* __restrict__ weight,
                                                                   const float* __restrict__ bias,
                                                                   const double* __restrict__ mean,
                                                                   const double* __restrict__ invstd,
                                                                   float* __restrict__ y, int64_t ldy) {
  const int rt = kBnThreads >> ctl;
  const int cx = threadIdx.x & ((1 << ctl) - 1), ry = threadIdx.x >> ctl;
  const int64_t c0 = (((int64_t)blockIdx.x << ctl) + cx) * V;
  if (c0 >= C) return;
  double m[V], is[V], w[V], b[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    m[j] = mean[c0 + j];
    is[j] = invstd[c0 + j];
    w[j] = weight ? (double)weight[c0 + j] : 1.0;
    b[j] = bias ? (double)bias[c0 + j] : 0.0;
  }
  for (int64_t r = (int64_t)blockIdx.y * rt + ry; r < M; r += (int64_t)gridDim.y * rt) {
    double v[V];
    bn_load<V>(x + r * ldx + c0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = fma((v[j] - m[j]) * is[j], w[j], b[j]);
    bn_store<V>(y + r * ldy + c0, v);
  }
}

// pass 1 of the backward: part[0][s][c] = sum g_y, part[1][s][c] = sum g_y xhat over stripe s;
// EVAL: g_x = g_y weight invstd needs no sums and is written here (g_x may be null)
template <int V, bool EVAL>
__global__ void __launch_bounds__(kBnThreads) bn_bwd_stats_kernel(
    int64_t M, int C, int ctl, int64_t rs, const float* __restrict__ x, int64_t ldx, const float* __restrict__ gy,
    int64_t ldgy, const float* __restrict__ weight, const double* __restrict__ mean,
    const double* __restrict__ invstd, float* __restrict__ gx, int64_t ldgx, double* __restrict__ part, int64_t R) {
  const int rt = kBnThreads >> ctl;
  const int cx = threadIdx.x & ((1 << ctl) - 1), ry = threadIdx.x >> ctl;
  const int64_t c0 = (((int64_t)blockIdx.x << ctl) + cx) * V;
  const bool live = c0 < C;
  const int64_t s = blockIdx.y;
  const int64_t r0 = s * rs, r1 = std::min<int64_t>(M, r0 + rs);
  double acc[2 * V];
#pragma unroll
  for (int j = 0; j < 2 * V; ++j) acc[j] = 0.0;
  if (live) {
    double m[V], is[V], k[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      m[j] = mean[c0 + j];
      is[j] = invstd[c0 + j];
      k[j] = (weight ? (double)weight[c0 + j] : 1.0) * is[j];
    }
    int64_t r = r0 + ry;
    for (; r + rt < r1; r += 2 * rt) {  // two rows of both inputs in flight
      double v[2][V], g[2][V];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        bn_load<V>(x + (r + u * rt) * ldx + c0, v[u]);
        bn_load<V>(gy + (r + u * rt) * ldgy + c0, g[u]);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          acc[j] += g[u][j];
          acc[V + j] = fma(g[u][j], (v[u][j] - m[j]) * is[j], acc[V + j]);
          if (EVAL) g[u][j] *= k[j];
        }
        if (EVAL && gx) bn_store<V>(gx + (r + u * rt) * ldgx + c0, g[u]);
      }
    }
    for (; r < r1; r += rt) {
      double v[V], g[V];
      bn_load<V>(x + r * ldx + c0, v);
      bn_load<V>(gy + r * ldgy + c0, g);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        acc[j] += g[j];
        acc[V + j] = fma(g[j], (v[j] - m[j]) * is[j], acc[V + j]);
        if (EVAL) g[j] *= k[j];
      }
      if (EVAL && gx) bn_store<V>(gx + r * ldgx + c0, g);
    }
  }
  bn_row_lane_sum<2 * V>(acc, ctl);
  if (live && ry == 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      part[(0 * R + s) * C + c0 + j] = acc[j];
      part[(1 * R + s) * C + c0 + j] = acc[V + j];
    }
  }
}

// g_bias = sum g_y, g_weight = sum g_y xhat from the stripe partials; both sums kept in fp64
// (sums[0][c], sums[1][c]) for the training backward's second pass
__global__ void __launch_bounds__(kBnThreads) bn_bwd_finalize_kernel(int C, int64_t R,
                                                                      const double* __restrict__ part,
                                                                      double* __restrict__ sums,
                                                                      float* __restrict__ g_weight,
                                                                      float* __restrict__ g_bias) {
  const int col = blockIdx.x * 16 + (threadIdx.x & 15);
  double sg, sgx;
  bn_sum_stripes(C, R, part, col, sg, sgx);
  if ((threadIdx.x >> 4) != 0 || col >= C) return;
  sums[col] = sg;
  sums[(int64_t)C + col] = sgx;
  if (g_bias) g_bias[col] = (float)sg;
  if (g_weight) g_weight[col] = (float)sgx;
}

// pass 2 of the training backward:
//   g_x = weight invstd / M * (M g_y - sum g_y - xhat sum(g_y xhat))
template <int V>
__global__ void __launch_bounds__(kBnThreads) bn_bwd_apply_kernel(
    int64_t M, int C, int ctl, const float* __restrict__ x, int64_t ldx, const float* __restrict__ gy,
    int64_t ldgy, const float* __restrict__ weight, const double* __restrict__ mean,
    const double* __restrict__ invstd, const double* __restrict__ sums, float* __restrict__ gx, int64_t ldgx) {
  const int rt = kBnThreads >> ctl;
  const int cx = threadIdx.x & ((1 << ctl) - 1), ry = threadIdx.x >> ctl;
  const int64_t c0 = (((int64_t)blockIdx.x << ctl) + cx) * V;
  if (c0 >= C) return;
  const double n = (double)M;
  double m[V], is[V], k[V], sg[V], sgx[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    m[j] = mean[c0 + j];
    is[j] = invstd[c0 + j];
    k[j] = (weight ? (double)weight[c0 + j] : 1.0) * is[j] / n;
    sg[j] = sums[c0 + j];
    sgx[j] = sums[(int64_t)C + c0 + j];
  }
  for (int64_t r = (int64_t)blockIdx.y * rt + ry; r < M; r += (int64_t)gridDim.y * rt) {
    double v[V], g[V];
    bn_load<V>(x + r * ldx + c0, v);
    bn_load<V>(gy + r * ldgy + c0, g);
#pragma unroll
    for (int j = 0; j < V; ++j) g[j] = k[j] * ((n * g[j] - sg[j]) - (v[j] - m[j]) * is[j] * sgx[j]);
    bn_store<V>(gx + r * ldgx + c0, g);
  }
}

struct BnGeom {
  bool vec;
  int ctl;
  unsigned col_blocks, apply_rows;
  int64_t R, rs;
};

// float4 accesses when C, every row pitch and every base pointer allow them, else scalar
BnGeom bn_geom(int64_t M, int C, bool vec) {
  BnGeom g;
  g.vec = vec;
  const int64_t cv = vec ? C / 4 : C;
  g.ctl = bn_ct_log2(cv);
  g.col_blocks = (unsigned)ceil_div(cv, int64_t(1) << g.ctl);
  const int rt = kBnThreads >> g.ctl;
  g.apply_rows = (unsigned)std::min<int64_t>(ceil_div(M, (int64_t)rt * 8), 32768);  // ~8 rows per thread
  g.R = bn_part_rows(M);
  g.rs = ceil_div(M, g.R);
  return g;
}

int bn_check(const char* who, int64_t M, int C, int training, double eps) {
  MVML_REQUIRE(M >= 1 && C >= 1, "%s: M and C must be >= 1 (got M=%lld, C=%d)", who, (long long)M, C);
  MVML_REQUIRE(!(training && M == 1), "%s: training needs more than 1 value per channel (M == 1)", who);
  MVML_REQUIRE(eps >= 0.0, "%s: eps must be >= 0", who);
  return MVML_OK;
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int64_t mvml_batchnorm1d_part_rows(int64_t M) { return bn_part_rows(M); }

extern "C" size_t mvml_batchnorm1d_workspace_size(int64_t M, int C) {
  if (M < 1 || C < 1) return 0;
  return carve_size((size_t)2 * bn_part_rows(M) * C * sizeof(double)) + carve_size((size_t)2 * C * sizeof(double));
}

extern "C" int mvml_batchnorm1d_fwd(int64_t M, int C, const float* x, int64_t ldx, const float* weight,
                                    const float* bias, int training, double momentum, double eps,
                                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                    float* y, int64_t ldy, double* save_mean, double* save_invstd,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (int rc = bn_check("batchnorm1d_fwd", M, C, training, eps)) return rc;
  MVML_REQUIRE(ldx >= C && ldy >= C, "batchnorm1d_fwd: row pitches must be >= C (ldx=%lld, ldy=%lld, C=%d)",
               (long long)ldx, (long long)ldy, C);
  MVML_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "batchnorm1d_fwd: momentum must be in [0, 1]");
  MVML_REQUIRE(x && y && save_mean && save_invstd, "batchnorm1d_fwd: x, y, save_mean and save_invstd are required");
  MVML_REQUIRE(training || (running_mean && running_var), "batchnorm1d_fwd: eval mode needs the running statistics");
  if (training && (!workspace || workspace_bytes < mvml_batchnorm1d_workspace_size(M, C))) {
    set_error("batchnorm1d_fwd: workspace too small");
    return MVML_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(x) && aligned16(y);
  const BnGeom g = bn_geom(M, C, vec);
  if (training) {
    double* part = static_cast<double*>(workspace);
    dim3 grid(g.col_blocks, (unsigned)g.R);
    if (vec)
      bn_fwd_stats_kernel<4><<<grid, kBnThreads, 0, st>>>(M, C, g.ctl, g.rs, x, ldx, part, g.R);
    else
      bn_fwd_stats_kernel<1><<<grid, kBnThreads, 0, st>>>(M, C, g.ctl, g.rs, x, ldx, part, g.R);
    if (int rc = check_launch("bn_fwd_stats_kernel")) return rc;
    bn_fwd_finalize_kernel<<<(unsigned)ceil_div(C, 16), kBnThreads, 0, st>>>(
        M, C, g.R, part, x, momentum, eps, running_mean, running_var, num_batches_tracked, save_mean, save_invstd);
    if (int rc = check_launch("bn_fwd_finalize_kernel")) return rc;
  } else {
    bn_eval_stats_kernel<<<(unsigned)ceil_div(C, 256), 256, 0, st>>>(C, running_mean, running_var, eps, save_mean,
                                                                     save_invstd);
    if (int rc = check_launch("bn_eval_stats_kernel")) return rc;
  }
  dim3 grid(g.col_blocks, g.apply_rows);
  if (vec)
    bn_fwd_apply_kernel<4><<<grid, kBnThreads, 0, st>>>(M, C, g.ctl, x, ldx, weight, bias, save_mean, save_invstd, y,
                                                        ldy);
  else
    bn_fwd_apply_kernel<1><<<grid, kBnThreads, 0, st>>>(M, C, g.ctl, x, ldx, weight, bias, save_mean, save_invstd, y,
                                                        ldy);
  return check_launch("bn_fwd_apply_kernel");
}

extern "C" int mvml_batchnorm1d_bwd(int64_t M, int C, const float* x, int64_t ldx, const float* weight,
                                    int training, const double* save_mean, const double* save_invstd,
                                    const float* g_y, int64_t ldgy, float* g_x, int64_t ldgx, float* g_weight,
                                    float* g_bias, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (int rc = bn_check("batchnorm1d_bwd", M, C, training, 0.0)) return rc;
  MVML_REQUIRE(ldx >= C && ldgy >= C && (!g_x || ldgx >= C),
               "batchnorm1d_bwd: row pitches must be >= C (ldx=%lld, ldgy=%lld, ldgx=%lld, C=%d)", (long long)ldx,
               (long long)ldgy, (long long)ldgx, C);
  MVML_REQUIRE(x && g_y && save_mean && save_invstd, "batchnorm1d_bwd: x, g_y, save_mean and save_invstd are required");
  if (!workspace || workspace_bytes < mvml_batchnorm1d_workspace_size(M, C)) {
    set_error("batchnorm1d_bwd: workspace too small");
    return MVML_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldgy % 4 == 0 && aligned16(x) && aligned16(g_y) &&
                   (!g_x || (ldgx % 4 == 0 && aligned16(g_x)));
  const BnGeom g = bn_geom(M, C, vec);
  Carver cv(workspace, workspace_bytes);
  double* part = cv.take<double>((size_t)2 * g.R * C);
  double* sums = cv.take<double>((size_t)2 * C);
  dim3 grid(g.col_blocks, (unsigned)g.R);
  auto stats = [&](auto v, auto eval) {
    bn_bwd_stats_kernel<decltype(v)::value, decltype(eval)::value><<<grid, kBnThreads, 0, st>>>(
        M, C, g.ctl, g.rs, x, ldx, g_y, ldgy, weight, save_mean, save_invstd, g_x, ldgx, part, g.R);
  };
  if (vec && training) stats(std::integral_constant<int, 4>{}, std::false_type{});
  else if (vec) stats(std::integral_constant<int, 4>{}, std::true_type{});
  else if (training) stats(std::integral_constant<int, 1>{}, std::false_type{});
  else stats(std::integral_constant<int, 1>{}, std::true_type{});
  if (int rc = check_launch("bn_bwd_stats_kernel")) return rc;
  bn_bwd_finalize_kernel<<<(unsigned)ceil_div(C, 16), kBnThreads, 0, st>>>(C, g.R, part, sums, g_weight, g_bias);
  if (int rc = check_launch("bn_bwd_finalize_kernel")) return rc;
  if (!training || !g_x) return MVML_OK;
  dim3 grid2(g.col_blocks, g.apply_rows);
  if (vec)
    bn_bwd_apply_kernel<4><<<grid2, kBnThreads, 0, st>>>(M, C, g.ctl, x, ldx, g_y, ldgy, weight, save_mean,
                                                         save_invstd, sums, g_x, ldgx);
  else
    bn_bwd_apply_kernel<1><<<grid2, kBnThreads, 0, st>>>(M, C, g.ctl, x, ldx, g_y, ldgy, weight, save_mean,
                                                         save_invstd, sums, g_x, ldgx);
  return check_launch("bn_bwd_apply_kernel");
}
