// Multi-label classification metrics of one batch on the device (mvml_multilabel_metrics):
// the reference's evaluate(labels, pred) (utils.py:109-135) without its device->host copy.
//
// Stage 1 (metrics_partial_kernel): one lane per row.  A row's label and prediction sets are
// 64-bit masks, one pair per 64 classes, and its counts are popcounts.  Every thread adds its
// rows' four fp64 terms in row order, the workgroup adds its threads' sums by a fixed tree, and
// the result goes to the workgroup's slot of the workspace.  The per-class tp / fp / fn / tn
// counts are integers: ballots over the wave, summed in LDS, one 64-bit integer atomic per
// class and workgroup.
// Stage 2 (metrics_final_kernel): one workgroup adds the (at most 256) partials by a fixed tree
// and writes sums[8].  No floating-point atomics and no hand-off between workgroups inside a
// launch: two runs on the same input give the same bits.
#include "common.h"

namespace mvml {

constexpr int kMetricThreads = 256;
constexpr int kMetricMaxBlocks = 256;  // one workgroup per CU; also stage 2's tree width
constexpr int kMetricSlots = 8;        // doubles per workgroup partial (5 used)

static int metric_blocks(int64_t B) {
  return (int)std::min<int64_t>(ceil_div(B, kMetricThreads), kMetricMaxBlocks);
}

// p = (z >= 0) on the bits: +0 .. +inf and -0.0 give 1; negatives, denormals included, and
// NaNs of either sign give 0 — whatever the denormal mode of the compare instruction.
__device__ __forceinline__ bool predict_bit(float z) {
  const uint32_t u = __float_as_uint(z);
  return u <= 0x7f800000u || u == 0x80000000u;
}

// Masks of classes [c0, c0 + nc) of one row (nc <= 64).
__device__ __forceinline__ void row_masks(const float* __restrict__ z, const float* __restrict__ y,
                                          int nc, uint64_t& ym, uint64_t& pm) {
  ym = 0;
  pm = 0;
  for (int c = 0; c < nc; ++c) {
    pm |= (uint64_t)predict_bit(z[c]) << c;
    ym |= (uint64_t)(y[c] >= 0.5f) << c;
  }
}

// Fixed-order sum over the workgroup; the result is valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from the previous call
  if (lane_id() == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(kMetricThreads)
metrics_partial_kernel(int64_t B, int C, const float* __restrict__ Z, int64_t ldz,
                       const float* __restrict__ Y, int64_t ldy, double* __restrict__ part,
                       unsigned long long* __restrict__ cls) {
  __shared__ double red[kMetricThreads / kWave];
  __shared__ unsigned long long cnt[4][kWave];
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * kMetricThreads;
  const int64_t first = (int64_t)blockIdx.x * kMetricThreads + threadIdx.x;
  const int64_t iters = ceil_div(B, stride);  // the same for every thread: ballots stay whole
  const int words = (C + 63) / 64;
  double s_jac = 0.0, s_pre = 0.0, s_rec = 0.0, s_f1 = 0.0, s_empty = 0.0;

  for (int w = 0; w < words; ++w) {
    const int c0 = w * 64, nc = min(64, C - c0);
    // this lane's class (c0 + lane) over the rows of its wave
    unsigned long long tp = 0, fp = 0, fn = 0, rows = 0;
    for (int64_t it = 0; it < iters; ++it) {
      const int64_t r = first + it * stride;
      const bool valid = r < B;
      uint64_t ym = 0, pm = 0;
      if (valid) row_masks(Z + r * ldz + c0, Y + r * ldy + c0, nc, ym, pm);
      if (w == 0 && valid) {
        int t = __popcll(ym & pm), u = __popcll(ym | pm), a = __popcll(ym), b = __popcll(pm);
        for (int w2 = 1; w2 < words; ++w2) {
          uint64_t y2, p2;
          row_masks(Z + r * ldz + w2 * 64, Y + r * ldy + w2 * 64, min(64, C - w2 * 64), y2, p2);
          t += __popcll(y2 & p2);
          u += __popcll(y2 | p2);
          a += __popcll(y2);
          b += __popcll(p2);
        }
        if (u > 0) s_jac += (double)t / (double)u; else s_empty += 1.0;
        if (b > 0) s_pre += (double)t / (double)b;
        if (a > 0) s_rec += (double)t / (double)a;
        if (a + b > 0) s_f1 += (double)(2 * t) / (double)(a + b);
      }
      rows += __popcll(__ballot(valid));
      for (int c = 0; c < nc; ++c) {
        const uint64_t by = __ballot((ym >> c) & 1), bp = __ballot((pm >> c) & 1);
        if (lane == c) {
          tp += __popcll(by & bp);
          fp += __popcll(~by & bp);
          fn += __popcll(by & ~bp);
        }
      }
    }
    if (threadIdx.x < kWave) {
#pragma unroll
      for (int k = 0; k < 4; ++k) cnt[k][threadIdx.x] = 0;
    }
    __syncthreads();
    if (lane < nc) {
      atomicAdd(&cnt[0][lane], tp);
      atomicAdd(&cnt[1][lane], fp);
      atomicAdd(&cnt[2][lane], fn);
      atomicAdd(&cnt[3][lane], rows - tp - fp - fn);
    }
    __syncthreads();
    {
      const int k = threadIdx.x >> 6;  // 256 threads: four counts x 64 classes
      if (lane < nc && cnt[k][lane] != 0) atomicAdd(&cls[(int64_t)k * C + c0 + lane], cnt[k][lane]);
    }
    __syncthreads();
  }

  const double v0 = block_sum(s_jac, red), v1 = block_sum(s_pre, red), v2 = block_sum(s_rec, red),
               v3 = block_sum(s_f1, red), v4 = block_sum(s_empty, red);
  if (threadIdx.x == 0) {
    double* p = part + (int64_t)blockIdx.x * kMetricSlots;
    p[0] = v0;
    p[1] = v1;
    p[2] = v2;
    p[3] = v3;
    p[4] = v4;
  }
}

// sums[0..3] = the four sums over the G partials, [4] = B, [5] = empty-union rows, [6..7] = 0.
__global__ void __launch_bounds__(kMetricMaxBlocks)
metrics_final_kernel(int64_t B, int G, const double* __restrict__ part, double* __restrict__ sums) {
  __shared__ double red[5][kMetricMaxBlocks];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][t] = t < G ? part[(int64_t)t * kMetricSlots + k] : 0.0;
  __syncthreads();
  for (int h = kMetricMaxBlocks / 2; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k][t] += red[k][t + h];
    }
    __syncthreads();
  }
  if (t < 8) sums[t] = t < 4 ? red[t][0] : t == 4 ? (double)B : t == 5 ? red[4][0] : 0.0;
}

}  // namespace mvml

using namespace mvml;

extern "C" size_t mvml_multilabel_metrics_workspace_size(int64_t B, int C) {
  if (B <= 0 || C < 1) return 0;
  return carve_size((size_t)metric_blocks(B) * kMetricSlots * sizeof(double));
}

extern "C" int mvml_multilabel_metrics(int64_t B, int C, const float* z, int64_t ldz, const float* y,
                                       int64_t ldy, double* sums, int64_t* class_counts,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  MVML_REQUIRE(B >= 0, "multilabel_metrics: negative batch size B = %lld", (long long)B);
  MVML_REQUIRE(C >= 1, "multilabel_metrics: C = %d classes (need at least 1)", C);
  MVML_REQUIRE(ldz >= C && ldy >= C,
               "multilabel_metrics: leading dimensions ldz = %lld, ldy = %lld below C = %d",
               (long long)ldz, (long long)ldy, C);
  const size_t need = mvml_multilabel_metrics_workspace_size(B, C);
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("multilabel_metrics: workspace too small (need %zu bytes)", need);
    return MVML_ERR_WORKSPACE;
  }
  MVML_REQUIRE(sums != nullptr, "multilabel_metrics: sums is required");
  MVML_REQUIRE(B == 0 || (z && y && class_counts), "multilabel_metrics: z, y and class_counts are required");
  hipStream_t st = as_stream(stream);
  const int G = B > 0 ? metric_blocks(B) : 0;
  double* part = static_cast<double*>(workspace);
  if (G > 0)
    metrics_partial_kernel<<<G, kMetricThreads, 0, st>>>(B, C, z, ldz, y, ldy, part,
                                                         reinterpret_cast<unsigned long long*>(class_counts));
  metrics_final_kernel<<<1, kMetricMaxBlocks, 0, st>>>(B, G, part, sums);
  return check_launch("multilabel_metrics");
}
