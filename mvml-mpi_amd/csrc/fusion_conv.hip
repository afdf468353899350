// Fusion head, Conv2d(12, 12, 3) + bias + ReLU over the (12, 3, W) attention cube of a molecule
// (model.py:27, 69; overview and sizes in fusion_common.h): forward and backward on the f32 matrix
// cores, the fixed-order sum of the backward's per-workgroup partials, and mvml_conv3_*.
#include "fusion_common.h"

namespace mvml {
namespace {

// Input gradient of conv3 (through the ReLU: g_pre = g_out * (out > 0)):
//   g_in[c][dy][x'] = sum_o sum_dx w[o][c][dy][dx] g_pre[o][x' - dx]   (0 <= x' - dx < W - 2)
// and per-workgroup weight / bias gradient partials over molecules [b0, b1):
//   part[blk][(o, c, dy, dx)] = sum_b sum_x g_pre[o][x] in[c][dy][x + dx], part[blk][2 * 1296 + o]
// (the row layout: kConvPart).
// Backward, one workgroup (6 waves) per range of molecules:
//  * input gradient: thread per column x' holds g_pre[o][x' - dx] (36 values) in registers and
//    accumulates the 36 (c, dy) outputs with scalar-loaded weights (1296 FMAs, no LDS in the
//    loop);
//  * weight / bias gradient on the f32 matrix cores: per molecule gW[o][n] += sum_x g_pre[o][x]
//    im2col[x][n] with n = (c, dy, dx) < 108 and n = 108 a column of ones (the bias), as
//    v_mfma_f32_16x16x4_f32 over 7 column tiles of 16; wave w owns the x-steps [64 w, 64 w + 64)
//    of every molecule, the fragments are per-lane LDS reads of the staged rows.  The six waves'
//    16 x 112 partial tiles are summed in fixed order at the end (deterministic, no atomics).
constexpr int kConvWaves = kConvThreads / 64;  // 6
__global__ void __launch_bounds__(kConvThreads, 2)  // the register budget of two waves per SIMD
conv3_bwd2_kernel(int64_t B, int W, int64_t per_block, const float* __restrict__ in,
                  const float* __restrict__ wgt, const float* __restrict__ out,
                  const float* __restrict__ g_out, float* __restrict__ g_in,
                  float* __restrict__ part) {
  __shared__ float s_in[kConvC * kConvH * kConvLd + 8];
  __shared__ float s_g[kConvO * kConvLd];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int Wo = W - 2;
  if (tid < 8) s_in[kConvC * kConvH * kConvLd + tid] = 0.f;  // reads past the last row: finite
  // the pad columns [W, kConvLd) of every row are read by the weight-gradient MFMA steps past
  // Wo (against a zero g_out): they must be finite (0 x NaN of stale LDS would be NaN)
  for (int i = tid; i < kConvC * kConvH * (kConvLd - W); i += kConvThreads)
    s_in[(i / (kConvLd - W)) * kConvLd + W + i % (kConvLd - W)] = 0.f;
  f32x4_t acc[kConvNT];
#pragma unroll
  for (int j = 0; j < kConvNT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // this lane's fixed fragment coordinates: A row o = lane & 15; B column n = 16 j + (lane & 15)
  const int lo = lane & 15, lk = lane >> 4;
  int boff[kConvNT];  // LDS offset of im2col(x = 0, n) (row (c, dy), column dx), or -1 / -2
#pragma unroll
  for (int j = 0; j < kConvNT; ++j) {
    const int n = 16 * j + lo;
    boff[j] = n < 108 ? (n / 3) * kConvLd + n % 3 : (n == 108 ? -1 : -2);
  }
  const int64_t b0 = (int64_t)blockIdx.x * per_block, b1 = min(B, b0 + per_block);
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // previous molecule's LDS reads done
    conv_stage(s_in, in + b * (int64_t)(kConvC * kConvH * W), kConvC * kConvH, W, tid);
    const float* go = g_out + b * (int64_t)(kConvO * Wo);
    const float* oo = out + b * (int64_t)(kConvO * Wo);
    {  // g_pre = g_out where out > 0, zero-padded rows; all loads before the stores
      constexpr int kIt = (kConvO * kConvLd + kConvThreads - 1) / kConvThreads;
      float gv[kIt], ov[kIt];
#pragma unroll
      for (int it = 0; it < kIt; ++it) {
        const int i = tid + it * kConvThreads, o = i / kConvLd, x = i % kConvLd;
        const bool ok = i < kConvO * kConvLd && x < Wo;
        gv[it] = ok ? go[o * Wo + x] : 0.f;
        ov[it] = ok ? oo[o * Wo + x] : 0.f;
      }
#pragma unroll
      for (int it = 0; it < kIt; ++it) {
        const int i = tid + it * kConvThreads;
        if (i < kConvO * kConvLd) s_g[i] = ov[it] > 0.f ? gv[it] : 0.f;
      }
    }
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);  // phases stay apart (registers)
    if (tid < W) {  // input gradient
      const int xp = tid;
      float g[kConvO][3];
#pragma unroll
      for (int o = 0; o < kConvO; ++o)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) g[o][dx] = xp - dx >= 0 ? s_g[o * kConvLd + xp - dx] : 0.f;
      float acc_in[kConvC * kConvH];
#pragma unroll
      for (int i = 0; i < kConvC * kConvH; ++i) acc_in[i] = 0.f;
#pragma unroll
      for (int o = 0; o < kConvO; ++o) {  // summed in (o, dx) order, o outer
        const float* w = wgt + o * (kConvC * kConvH * 3);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
          for (int cd = 0; cd < kConvC * kConvH; ++cd)
            acc_in[cd] = fmaf(w[cd * 3 + dx], g[o][dx], acc_in[cd]);
      }
      float* dst = g_in + b * (int64_t)(kConvC * kConvH * W) + xp;
#pragma unroll
      for (int cd = 0; cd < kConvC * kConvH; ++cd) dst[cd * W] = acc_in[cd];
    }
    __builtin_amdgcn_sched_barrier(0);
    // weight / bias gradient: x-steps of 4 columns, wave w takes steps [16 w, 16 w + 16)
    for (int ks = 16 * wid; ks < 16 * wid + 16; ++ks) {
      const int x = 4 * ks + lk;
      const float av = lo < kConvO ? s_g[lo * kConvLd + x] : 0.f;  // 0 past Wo (padding)
#pragma unroll
      for (int j = 0; j < kConvNT; ++j) {
        const float bv = boff[j] >= 0 ? s_in[boff[j] + x] : (boff[j] == -1 ? 1.f : 0.f);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
      }
    }
  }
  // fixed-order reduction of the six waves' 16 x 112 tiles: C[i][n], i = 4 (lane >> 4) + r
  __syncthreads();
  float* red = s_in;  // 6 x 16 x 112 floats = 42 KB <= s_in
#pragma unroll
  for (int j = 0; j < kConvNT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wid * 16 + 4 * lk + r) * 112 + 16 * j + lo] = acc[j][r];
  __syncthreads();
  for (int i = tid; i < kConvO * 109; i += kConvThreads) {
    const int o = i / 109, n = i % 109;
    float s = 0.f;
    for (int w = 0; w < kConvWaves; ++w) s += red[(w * 16 + o) * 112 + n];
    if (n < 108) part[(int64_t)blockIdx.x * kConvPart + o * 108 + n] = s;
    else part[(int64_t)blockIdx.x * kConvPart + 2 * kConvWg + o] = s;
  }
}

// Forward on the matrix cores (the weight / bias fragments and the im2col offsets are written out
// here, in conv3_bwd2_kernel and in the fused kernels: shared helpers for them compile to other
// instruction streams in all of these): out[o][x] = ReLU(b[o] + sum_k W[o][k] im2col[k][x]), k = (c, dy,
// dx) < 108 in 27 steps of v_mfma_f32_16x16x4_f32, M = 12 output channels (one 16-row tile), wave w
// the columns [64 w, 64 w + 64); the weight fragments (27 per lane) are loaded once per
// workgroup, the im2col operand is a per-lane LDS read of the staged rows.  (A per-thread VALU
// loop got its 1296 weights as 81 serialised scalar loads per molecule.)
__global__ void __launch_bounds__(kConvThreads, 3)  // two workgroups per CU (3 waves per SIMD)
conv3_fwd3_kernel(int64_t B, int W, int64_t per_block, const float* __restrict__ in,
                  const float* __restrict__ wgt, const float* __restrict__ bias,
                  float* __restrict__ out) {
  __shared__ float s_in[kConvC * kConvH * kConvLd + 8];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lo = lane & 15, lk = lane >> 4;
  const int Wo = W - 2;
  float wfr[27];
#pragma unroll
  for (int ks = 0; ks < 27; ++ks) wfr[ks] = lo < kConvO ? wgt[lo * 108 + 4 * ks + lk] : 0.f;
  float bo[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bo[r] = 4 * lk + r < kConvO ? bias[4 * lk + r] : 0.f;
  if (tid < 8) s_in[kConvC * kConvH * kConvLd + tid] = 0.f;
  const int64_t b0 = (int64_t)blockIdx.x * per_block, b1 = min(B, b0 + per_block);
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // previous molecule's LDS reads done
    conv_stage(s_in, in + b * (int64_t)(kConvC * kConvH * W), kConvC * kConvH, W, tid);
    __syncthreads();
    f32x4_t acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 27; ++ks) {
      const int k = 4 * ks + lk;  // im2col row: (c, dy) = k / 3, shift dx = k % 3
      const int koff = (k / 3) * kConvLd + k % 3;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float bv = s_in[koff + 64 * wid + 16 * ct + lo];  // columns >= Wo: discarded
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wfr[ks], bv, acc[ct], 0, 0, 0);
      }
    }
    float* ob = out + b * (int64_t)(kConvO * Wo);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int x = 64 * wid + 16 * ct + lo;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 4 * lk + r;
        if (o < kConvO && x < Wo) ob[o * Wo + x] = fmaxf(acc[ct][r] + bo[r], 0.f);
      }
    }
  }
}

// Fixed-order sum of the per-workgroup partials: out[i] = sum_blk part[blk * stride + i].
__global__ void partial_sum_kernel(int nblk, int count, int stride, const float* __restrict__ part,
                                   float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  // eight independent partial sums keep eight loads in flight (the loop is latency-bound);
  // the fixed combination order keeps the result deterministic
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto at = [&](int r) { return part[(int64_t)r * stride + i]; };
  int r = 0;
  for (; r + 8 <= nblk; r += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += at(r + u);
  }
  for (; r < nblk; ++r) a[0] += at(r);
  out[i] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

}  // namespace

int sum_conv_partials(int nblk, const float* part, float* g_weight, float* g_bias, hipStream_t st) {
  partial_sum_kernel<<<(unsigned)ceil_div(kConvWg, 256), 256, 0, st>>>(nblk, kConvWg, kConvPart, part,
                                                                       g_weight);
  const int rc = check_launch("partial_sum_kernel(w)");
  if (rc) return rc;
  partial_sum_kernel<<<1, 64, 0, st>>>(nblk, kConvO, kConvPart, part + 2 * kConvWg, g_bias);
  return check_launch("partial_sum_kernel(b)");
}

}  // namespace mvml

using namespace mvml;

static int64_t conv3_blocks(int64_t B) { return std::min<int64_t>(B, 512); }  // 2 per CU

extern "C" int mvml_conv3_fwd(int64_t B, int C, int O, int W, const float* in, const float* weight,
                              const float* bias, float* out, void* stream) {
  clear_error();
  MVML_REQUIRE(C == kConvC && O == kConvO && W >= 3 && W <= 384, "conv3_fwd: C = O = 12, 3 <= W <= 384");
  if (B == 0) return MVML_OK;
  const int64_t nblk = conv3_blocks(B), per = ceil_div(B, nblk);
  conv3_fwd3_kernel<<<(unsigned)ceil_div(B, per), kConvThreads, 0, as_stream(stream)>>>(
      B, W, per, in, weight, bias, out);
  return check_launch("conv3_fwd_kernel");
}

extern "C" size_t mvml_conv3_bwd_workspace_size(int64_t B) {
  return carve_size((size_t)conv3_blocks(B > 0 ? B : 1) * kConvPart * sizeof(float));
}

extern "C" int mvml_conv3_bwd(int64_t B, int C, int O, int W, const float* in, const float* weight,
                              const float* out, const float* g_out, float* g_in, float* g_weight,
                              float* g_bias, void* workspace, size_t workspace_bytes,
                              void* stream) {
  clear_error();
  MVML_REQUIRE(C == kConvC && O == kConvO && W >= 3 && W <= 384, "conv3_bwd: C = O = 12, 3 <= W <= 384");
  if (B == 0) return MVML_OK;
  if (!workspace || workspace_bytes < mvml_conv3_bwd_workspace_size(B)) {
    set_error("conv3_bwd: workspace of mvml_conv3_bwd_workspace_size bytes required");
    return MVML_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int64_t nblk = conv3_blocks(B), per = ceil_div(B, nblk);
  const int64_t used = ceil_div(B, per);
  float* part = static_cast<float*>(workspace);
  conv3_bwd2_kernel<<<(unsigned)used, kConvThreads, 0, st>>>(B, W, per, in, weight, out, g_out,
                                                             g_in, part);
  const int rc = check_launch("conv3_bwd_kernel");
  if (rc) return rc;
  return sum_conv_partials((int)used, part, g_weight, g_bias, st);
}
