// Operand preparation of the split-fp16 GEMMs (gemm_f32.hip, gemm_smallk.hip): operand and
// per-row |max| bits (the scales), the interleaved fp16 pre-splits of an operand, and column sums.
#include <algorithm>

#include "common.h"
#include "gemm_common.h"

namespace mvml {
namespace {

// Column sums, stage 1: each thread owns one column of a row chunk; eight independent partial
// sums keep eight loads in flight per lane (the loop is otherwise latency-bound).
__global__ void colsum_partial_kernel(int64_t M, int64_t N, const float* __restrict__ X,
                                      int64_t ldx, int64_t rows_per, float* __restrict__ part) {
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= N) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int64_t r = r0;
  for (; r + 8 <= r1; r += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += X[(r + j) * ldx + col];
  }
  for (; r < r1; ++r) s[0] += X[r * ldx + col];
  part[(int64_t)blockIdx.y * N + col] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// out[col] = beta out[col] + alpha sum_z part[z ld + col]: a workgroup per 16 columns, 16 stripes of
// the S partials per column (four accumulators each, loads in flight), a fixed-order LDS tree —
// deterministic.  (A thread per column walking all S ~ 1024 partials took 20-70 us.)
__global__ void __launch_bounds__(256) colsum_final_kernel(int64_t N, int S, const float* __restrict__ part,
                                                           int64_t ld, float alpha, float beta,
                                                           float* __restrict__ out) {
  const int c = threadIdx.x & 15, stripe = threadIdx.x >> 4;
  const int64_t col = (int64_t)blockIdx.x * 16 + c;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (col < N) {
    int z = stripe;
    for (; z + 48 < S; z += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] += part[(int64_t)(z + 16 * u) * ld + col];
    }
    for (; z < S; z += 16) a[0] += part[(int64_t)z * ld + col];
  }
  __shared__ float red[16][17];
  red[stripe][c] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  for (int h = 8; h > 0; h >>= 1) {
    if (stripe < h) red[stripe][c] += red[stripe + h][c];
    __syncthreads();
  }
  if (stripe == 0 && col < N) out[col] = (beta != 0.f ? beta * out[col] : 0.f) + alpha * red[0][c];
}

// |max| of a stored rows x cols fp32 matrix (row pitch ld) folded into *out as float bits:
// non-negative float bits order like the values, so an unsigned atomicMax per workgroup is
// order-independent (deterministic).  Four independent rows in flight per thread.
__global__ void __launch_bounds__(256) absmax_kernel(int64_t rows, int64_t cols,
                                                     const float* __restrict__ P, int64_t ld,
                                                     int vec, uint32_t* __restrict__ out) {
  float m[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t rs = gridDim.y;
  if (vec) {  // cols % 4 == 0, ld % 4 == 0, 16-B aligned base: c indexes float4 columns
    if (c < cols / 4) {
      int64_t r = blockIdx.y;
      for (; r + 3 * rs < rows; r += 4 * rs) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(P + (r + u * rs) * ld + 4 * c);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          m[u] = fmaxf(m[u], fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w))));
      }
      for (; r < rows; r += rs) {
        const float4 v = *reinterpret_cast<const float4*>(P + r * ld + 4 * c);
        m[0] = fmaxf(m[0], fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
      }
    }
  } else if (c < cols) {
    for (int64_t r = blockIdx.y; r < rows; r += rs) m[0] = fmaxf(m[0], fabsf(P[r * ld + c]));
  }
  float v = wave_max(fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3])));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(out, __float_as_uint(v));
  }
}

// |max| of a contiguous run of n floats (a matrix with ld == cols, or one row): grid-stride over
// float4s (vec) or floats, 4 loads in flight per thread, one atomicMax per workgroup.  The
// column-parallel absmax_kernel leaves all but `cols` lanes of a workgroup idle, which for the
// GAT layers' max-of-row-maxima (N x 1) was 1 live lane in 256: ~0.4 ms per 1.75 M atoms.
__global__ void __launch_bounds__(256) absmax_flat_kernel(int64_t n, const float* __restrict__ P,
                                                          int vec, uint32_t* __restrict__ out) {
  float m[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (vec) {
    const int64_t n4 = n / 4;
    const float4* P4 = reinterpret_cast<const float4*>(P);
    for (; i + 3 * stride < n4; i += 4 * stride) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = P4[i + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        m[u] = fmaxf(m[u], fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w))));
    }
    for (; i < n4; i += stride) {
      const float4 v = P4[i];
      m[0] = fmaxf(m[0], fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
  } else {
    for (; i < n; i += stride) m[0] = fmaxf(m[0], fabsf(P[i]));
  }
  float v = wave_max(fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3])));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(out, __float_as_uint(v));
  }
}

// Per-row |max| bits: a group of 2^lg lanes per row (float4 columns when vec), butterfly max;
// one writer per row (accumulate: max with the stored bits), so no atomics.
__global__ void __launch_bounds__(256) absmax_rows_kernel(int64_t rows, int64_t cols,
                                                          const float* __restrict__ P, int64_t ld,
                                                          int vec, int lg, int accumulate,
                                                          uint32_t* __restrict__ out) {
  const int L = 1 << lg;
  const int64_t groups = (int64_t)gridDim.x * (256 >> lg);
  const int sub = threadIdx.x & (L - 1);
  for (int64_t row = (int64_t)blockIdx.x * (256 >> lg) + (threadIdx.x >> lg); row < rows; row += groups) {
    const float* p = P + row * ld;
    float m = 0.f;
    if (vec) {
      for (int64_t c = sub; c < cols / 4; c += L) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4 * c);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
      }
    } else {
      for (int64_t c = sub; c < cols; c += L) m = fmaxf(m, fabsf(p[c]));
    }
    for (int o = L / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (sub == 0) {
      uint32_t b = __float_as_uint(m);
      if (accumulate) b = max(b, out[row]);
      out[row] = b;
    }
  }
}

// Interleaved pre-split of a K-contiguous operand for the 128x128 kernel's BPS path: every
// 8-value k group becomes its 8 scaled high fp16 halves then its 8 low halves (split2h8's h, l),
// 32 B in place of the group's 32 B of fp32, so the LDS-DMA staging and the swizzle are unchanged
// and a fragment read yields the two MFMA operands ready-made.  K % 8 == 0 (host).
__global__ void __launch_bounds__(256) split_f16x2_il_kernel(int64_t rows, int64_t groups,
                                                             const float* __restrict__ P, int64_t ld,
                                                             const uint32_t* __restrict__ amax,
                                                             float* __restrict__ out) {
  const float sc = pow2f(amax_shift(*amax));
  const int64_t total = rows * groups;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / groups, c = 8 * (e - r * groups);
    const float* src = P + r * ld + c;
    bf16x8 h, l;
    split2h8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), sc, h, l);
    float* dst = out + r * ld + c;
    *reinterpret_cast<float4*>(dst) = __builtin_bit_cast(float4, h);
    *reinterpret_cast<float4*>(dst + 4) = __builtin_bit_cast(float4, l);
  }
}

// Interleaved-by-4 pre-split for the 256x256 kernels (BPS 2): every 4-value group of a row
// becomes [4 scaled high fp16 | 4 low fp16] = 16 B in place of its 16 B of fp32, so the image
// has the operand's own float indexing (any layout, K-contiguous or K-major) and a staged piece
// is one 16-B load, stored to the LDS planes as it is (split2h of the kernel's own staging).
__global__ void __launch_bounds__(256) split_f16x2_il4_kernel(int64_t rows, int64_t cols4,
                                                              const float* __restrict__ P, int64_t ld,
                                                              const uint32_t* __restrict__ amax,
                                                              float* __restrict__ out) {
  const float sc = pow2f(amax_shift(*amax));
  const int64_t total = rows * cols4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / cols4, c = 4 * (e - r * cols4);
    uint2 h, l;
    split2h(*reinterpret_cast<const float4*>(P + r * ld + c), sc, h, l);
    *reinterpret_cast<float4*>(out + r * ld + c) =
        make_float4(__uint_as_float(h.x), __uint_as_float(h.y), __uint_as_float(l.x), __uint_as_float(l.y));
  }
}

int absmax_rows_launch(int64_t rows, int64_t cols, const float* P, int64_t ld, uint32_t* out,
                       bool accumulate, hipStream_t st) {
  if (rows <= 0) return MVML_OK;
  if (cols <= 0) {
    if (accumulate) return MVML_OK;
    if (hipMemsetAsync(out, 0, rows * sizeof(uint32_t), st) != hipSuccess) {
      set_error("absmax_rows: hipMemsetAsync failed");
      return MVML_ERR_LAUNCH;
    }
    return MVML_OK;
  }
  const int vec = (cols % 4 == 0) && (ld % 4 == 0) && ((uintptr_t)P % 16 == 0);
  const int64_t units = vec ? cols / 4 : cols;
  int lg = 0;
  while ((1 << lg) < units && lg < 6) ++lg;  // lanes per row: enough for one unit each, <= 64
  const int64_t per_block = 256 >> lg;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(rows, per_block), 16384));
  absmax_rows_kernel<<<blocks, 256, 0, st>>>(rows, cols, P, ld, vec, lg, accumulate ? 1 : 0, out);
  return check_launch("absmax_rows_kernel");
}

int colsum_splits(int64_t M, int64_t N) {
  const int64_t colblocks = ceil_div(N, 256);
  int64_t s = ceil_div(2048, colblocks);
  s = std::min<int64_t>(s, ceil_div(M, 64));
  return (int)std::max<int64_t>(1, std::min<int64_t>(s, 4096));
}

}  // namespace

int split_il_launch(int64_t rows, int64_t K, const float* P, const uint32_t* amax, float* out,
                    hipStream_t st) {
  const int64_t total = rows * (K / 8);
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(total, 256), 4096));
  split_f16x2_il_kernel<<<blocks, 256, 0, st>>>(rows, K / 8, P, K, amax, out);
  return check_launch("split_f16x2_il_kernel");
}

int absmax_launch(int64_t rows, int64_t cols, const float* P, int64_t ld, uint32_t* out,
                  bool accumulate, hipStream_t st) {
  if (!accumulate && hipMemsetAsync(out, 0, sizeof(uint32_t), st) != hipSuccess) {
    set_error("absmax: hipMemsetAsync failed");
    return MVML_ERR_LAUNCH;
  }
  if (rows <= 0 || cols <= 0) return MVML_OK;
  if (ld == cols || rows == 1) {  // contiguous: one flat pass (also bounds the atomics at ~1 K)
    const int64_t n = rows * cols;
    const int fvec = (n % 4 == 0) && ((uintptr_t)P % 16 == 0);
    const unsigned blocks =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(fvec ? n / 4 : n, 256 * 4), 1024));
    absmax_flat_kernel<<<blocks, 256, 0, st>>>(n, P, fvec, out);
    return check_launch("absmax_flat_kernel");
  }
  const int vec = (cols % 4 == 0) && (ld % 4 == 0) && ((uintptr_t)P % 16 == 0);
  const int64_t cx = ceil_div(vec ? cols / 4 : cols, 256);
  // ~1 K workgroups (each ends with ONE atomicMax on the single output word: a word takes ~90
  // atomics per us, so the round-4 8 K workgroups spent ~90 us of a 150 us pass on them); each
  // thread walks its column down rows 4 at a time, enough loads in flight for HBM rate
  const int64_t ry = std::max<int64_t>(1, std::min<int64_t>(ceil_div(rows, 4), ceil_div(1024, cx)));
  absmax_kernel<<<dim3((unsigned)cx, (unsigned)ry), 256, 0, st>>>(rows, cols, P, ld, vec, out);
  return check_launch("absmax_kernel");
}

int colsum_final_launch(int64_t N, int S, const float* part, int64_t ld, float alpha, float beta,
                        float* out, hipStream_t st, const char* what) {
  colsum_final_kernel<<<(unsigned)ceil_div(N, 16), 256, 0, st>>>(N, S, part, ld, alpha, beta, out);
  return check_launch(what);
}

}  // namespace mvml

using namespace mvml;

extern "C" int mvml_split_f16x2_il4(int64_t rows, int64_t cols, const float* P, int64_t ld,
                                    const uint32_t* amax, float* out, void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && cols >= 0 && cols % 4 == 0 && ld % 4 == 0 && ld >= cols && amax &&
                   out && ((uintptr_t)P % 16) == 0 && ((uintptr_t)out % 16) == 0,
               "split_f16x2_il4: bad shape / alignment");
  if (rows == 0 || cols == 0) return MVML_OK;
  const int64_t total = rows * (cols / 4);
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(total, 256), 8192);
  split_f16x2_il4_kernel<<<blocks, 256, 0, as_stream(stream)>>>(rows, cols / 4, P, ld, amax, out);
  return check_launch("split_f16x2_il4_kernel");
}

extern "C" int mvml_absmax_rows_f32(int64_t rows, int64_t cols, const float* P, int64_t ld,
                                    uint32_t* out, int accumulate, void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && cols >= 0 && (rows == 0 || ld >= cols) && out, "absmax_rows: bad shape");
  return absmax_rows_launch(rows, cols, P, ld, out, accumulate != 0, as_stream(stream));
}

extern "C" int mvml_absmax_f32(int64_t rows, int64_t cols, const float* P, int64_t ld,
                               uint32_t* out, int accumulate, void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && cols >= 0 && (rows == 0 || ld >= cols) && out, "absmax: bad shape");
  return absmax_launch(rows, cols, P, ld, out, accumulate != 0, as_stream(stream));
}

extern "C" size_t mvml_colsum_workspace_size(int64_t M, int64_t N) {
  return carve_size((size_t)colsum_splits(M, N) * N * sizeof(float));
}

extern "C" int mvml_colsum_f32(int64_t M, int64_t N, const float* X, int64_t ldx, float alpha,
                               float beta, float* out, void* workspace, size_t workspace_bytes,
                               void* stream) {
  clear_error();
  MVML_REQUIRE(M >= 0 && N >= 0 && ldx >= N, "colsum: bad shape");
  if (N == 0) return MVML_OK;
  if (workspace_bytes < mvml_colsum_workspace_size(M, N) || !workspace) {
    set_error("colsum: workspace too small");
    return MVML_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int S = colsum_splits(M, N);
  const int64_t rows_per = ceil_div(M > 0 ? M : 1, S);
  float* part = static_cast<float*>(workspace);
  dim3 g1((unsigned)ceil_div(N, 256), (unsigned)S);
  colsum_partial_kernel<<<g1, 256, 0, st>>>(M, N, X, ldx, rows_per, part);
  return colsum_final_launch(N, S, part, N, alpha, beta, out, st, "colsum");
}
