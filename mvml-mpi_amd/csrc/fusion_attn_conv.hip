// Fusion head, token attention and Conv2d in one kernel per direction (overview in
// fusion_common.h), and mvml_attn_conv_*.
#include "fusion_common.h"
#include "dropout.h"

namespace mvml {
namespace {

// The (12, 3, 384) attention cube of a molecule is formed in LDS and consumed there by the
// convolution: it never makes the HBM round trip between the attention and the Conv2d (forward:
// 55 KB written + read per molecule; backward: the cube read, its gradient written and read
// again).  One workgroup of 12 waves per run of molecules, wave h = head h; the attention
// arithmetic is token_attn_fold_fwd / _bwd's (same operation order, so the cube and every g_pv
// element are bit-identical to the unfused pair), the convolution conv3_fwd3 / conv3_bwd2's
// with the column tiles spread over 12 waves.  The backward recomputes the cube as P V (bitwise
// the forward's values) instead of reading a saved copy, and sums the keys' gradient over heads
// as twelve wave partials added in head order (the unfused kernel's order).
constexpr int kFuseWaves = 12;  // = kConvC heads
constexpr int kFuseThreads = 64 * kFuseWaves;
constexpr int kFuseW = 64 * kDkVpl;              // 384 columns
constexpr int kFuseCube = kConvC * kConvH * kConvLd + 8;  // cube rows (h, t) + a zero tail
constexpr int kFuseG = kConvO * kConvLd;          // g_pre rows o
static_assert(kFuseW <= kConvLd - 1, "one pad column per cube row");

// att rows (h, a) = sum_c p_ac v_c into the LDS cube (row stride kConvLd at every width; the
// columns >= W of a row are not written)
template <bool kMask, int kV>
__device__ __forceinline__ void fold_att_lds(const float (&p)[NT][NT], const float (&v)[NT][kV],
                                             float* s_rows, int lane, int W) {
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      float o = 0.f;
#pragma unroll
      for (int c = 0; c < NT; ++c) o = fmaf(p[a][c], v[c][i], o);
      if (col_ok<kMask, kV>(lane, i, W)) s_rows[a * kConvLd + lane + 64 * i] = o;
    }
}

template <bool kMask, int kV>
__device__ __forceinline__ void load_rows3(const float* __restrict__ base, int64_t ld, int lane,
                                           float (&r)[NT][kV], int W) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < kV; ++i) r[t][i] = col_ld<kMask, kV>(base, t * ld, lane, i, W);
}

// kMask = false: W = 384 at compile time (dk is not read); kMask = true: W = dk, a multiple of 4
// in [16, 384].  The cube keeps its 385-float row stride, so a wave's column tiles and every
// LDS offset are the 384 instance's; waves whose tile starts at or past W - 2 skip the MFMA steps.
template <bool kMask, int kV>
__global__ void __launch_bounds__(kFuseThreads, 3)  // one workgroup per CU
attn_conv_fwd_kernel(int64_t B, int64_t per_block, const float* __restrict__ pv, int64_t ld,
                     const float* __restrict__ x, int64_t ldx, float scale,
                     const float* __restrict__ wgt, const float* __restrict__ bias,
                     float* __restrict__ P, float* __restrict__ out, uint32_t drop_thr,
                     float drop_scale, uint64_t drop_seed, int dk) {
  constexpr int H = kConvC;
  const int W = kMask ? dk : kFuseW, Wo = W - 2;
  const int64_t HD = (int64_t)H * W;
  __shared__ float s_in[kFuseCube];
  const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
  const int lo = lane & 15, lk = lane >> 4;
  float wfr[27];  // fragments and im2col offsets written out as in conv3_fwd3_kernel (see there)
#pragma unroll
  for (int ks = 0; ks < 27; ++ks) wfr[ks] = lo < kConvO ? wgt[lo * 108 + 4 * ks + lk] : 0.f;
  float bo[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bo[r] = 4 * lk + r < kConvO ? bias[4 * lk + r] : 0.f;
  if (tid < 8) s_in[kConvC * kConvH * kConvLd + tid] = 0.f;
  const int64_t b0 = (int64_t)blockIdx.x * per_block, b1 = min(B, b0 + per_block);
  // head h's rows of molecule b: keys (the LayerNorm rows), p and v; the next molecule's are
  // loaded while this one's convolution runs
  float k[NT][kV], q[NT][kV], v[NT][kV];
  auto load = [&](int64_t b) {
    load_rows3<kMask>(x + b * NT * ldx, ldx, lane, k, W);
    load_rows3<kMask>(pv + b * NT * ld + (int64_t)h * W, ld, lane, q, W);
    load_rows3<kMask>(pv + b * NT * ld + HD + (int64_t)h * W, ld, lane, v, W);
  };
  if (b0 < b1) load(b0);
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // the previous molecule's convolution reads of the cube are done
    {
      float p[NT][NT];
      fold_scores(q, k, scale, p);
      fold_att_lds<kMask>(p, v, s_in + h * NT * kConvLd, lane, W);
      if (lane < NT * NT) {  // written out as in token_attn_fold_fwd_kernel (see there)
        float pvv = p[0][0];
#pragma unroll
        for (int e = 1; e < NT * NT; ++e) pvv = lane == e ? p[e / NT][e % NT] : pvv;
        P[(b * H + h) * NT * NT + lane] = pvv;
      }
    }
    if (b + 1 < b1) load(b + 1);
    __syncthreads();
    // Conv2d + bias + ReLU on the matrix cores (conv3_fwd3_kernel): wave h the column tiles
    // [32 h, 32 h + 32)
    if (kMask && 32 * h >= Wo) continue;  // no output column in this wave's tiles (wave-uniform)
    f32x4_t acc[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 27; ++ks) {
      const int kk = 4 * ks + lk;
      const int koff = (kk / 3) * kConvLd + kk % 3;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float bv = s_in[koff + 32 * h + 16 * ct + lo];  // columns >= Wo: discarded
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wfr[ks], bv, acc[ct], 0, 0, 0);
      }
    }
    float* ob = out + b * (int64_t)(kConvO * Wo);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int xx = 32 * h + 16 * ct + lo;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 4 * lk + r;
        if (o < kConvO && xx < Wo) {
          float y = fmaxf(acc[ct][r] + bo[r], 0.f);
          if (drop_thr)  // the Dropout after the ReLU (model.py:36), mvml_dropout_fwd's mask
            y = dropout_u32(drop_seed, b * (int64_t)(kConvO * Wo) + o * Wo + xx) >= drop_thr ? y * drop_scale
                                                                                               : 0.f;
          ob[o * Wo + xx] = y;
        }
      }
    }
  }
}

// Backward of attn_conv_fwd, one molecule per loop trip, its inputs prefetched one molecule
// ahead by LDS-DMA (global_load_lds_dwordx4: no registers, the loads of molecule b + 1 fly
// while molecule b computes):
//   (A) wait for molecule b's staged g_out / out / v / P, barrier;
//   (B) the cube recomputed as P v into LDS (wave h: head h);
//   (C) Conv2d weight gradient on the matrix cores (conv3_bwd2's MFMA steps, wave w the x-steps
//       [8 w, 8 w + 8)) and the bias row sums, g_pre = g_out (out > 0) read from the staged rows;
//   (D) the cube's gradient (conv3_bwd2's VALU loop; threads t and t + 384 the (c, dy) rows
//       [0, 18) / [18, 36) of column t) in registers; barrier, then the cube gradient is stored
//       over the cube, each wave moves its head's v / P rows to registers, molecule b + 1's
//       g_out / out start into their (now free) staging rows and the wave's query / key loads
//       are issued; barrier, then molecule b + 1's v / P start;
//   (E) the attention backward of head h (token_attn_fold_bwd): g_pv stores, the keys'
//       gradient partial over head h's own cube rows, then the twelve partials in head order.
// Staging (one __shared__ array): cube [36 x 385 + 8] | g_out [18 KB] | out [18 KB] | v [3 x
// 4608] | P [108 + pad], each region a whole number of 1-KB DMA pieces.
// At a width W < 384 (kMask) the layout, the piece counts and every wave's share of the pieces
// stay the 384 ones: a molecule's g_out / out block (12 (W - 2) floats) and each v row (12 W
// floats) fill the front of their regions, and a lane whose float4 would start past the end of
// its source re-reads the source's last float4 (an aligned, in-range address: 48 (W - 2) and
// 48 W bytes are multiples of 16) into LDS words nothing reads.
constexpr int kStG = 18;                       // 1-KB pieces of a molecule's g_out (4584 floats)
constexpr int kStV = 54;                       // v: 3 rows x 4608 floats
constexpr int kStVP = kStV + 1;                // + P (108 floats)
constexpr int kOffG = ((kFuseCube * 4 + 1023) / 1024) * 256;  // float offsets of the regions
constexpr int kOffO = kOffG + kStG * 256;
constexpr int kOffV = kOffO + kStG * 256;
constexpr int kOffP = kOffV + kStV * 256;
constexpr int kBwdLds = kOffP + 256;
constexpr int kStVRow = (kStV / NT) * 256;    // LDS stride of the staged v rows (= 12 x 384)
static_assert(kBwdLds * 4 <= 160 * 1024, "backward staging fits the CU's LDS");
static_assert(kConvO * (kFuseW - 2) <= kStG * 256, "g_out rows fit their staging");

// a wave-uniform pointer held in SGPRs (so a global_load_lds takes the saddr + 32-bit lane
// offset form instead of a 64-bit address per lane)
__device__ __forceinline__ const float* uniform_ptr(const float* p) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ void glds16(const float* src, float* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// molecule b's g_out and out rows (contiguous 4584-float blocks) into their staging rows:
// pieces h and h + 12 of each (18 pieces), lanes past the block re-read its last float4
template <bool kMask>
__device__ __forceinline__ void stage_go(const float* __restrict__ g_out, const float* __restrict__ out,
                                         int64_t b, float* lds, int h, int lane, int W) {
  const int n = kConvO * ((kMask ? W : kFuseW) - 2);
  const int64_t base = b * (int64_t)n;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int piece = h + kFuseWaves * k;
    if (piece < kStG) {
      const int off = min(piece * 256 + 4 * lane, n - 4);
      glds16(g_out + base + off, lds + kOffG + piece * 256);
      glds16(out + base + off, lds + kOffO + piece * 256);
    }
  }
}

// molecule b's v rows (3 x 4608 floats of pv at column H dk) and P (108 floats): wave h issues
// pieces 5 h .. 5 h + 4 of the 55; wave 11's five (and nothing else) repeat the P piece — every
// wave issues exactly five, so the compiler's wait for the query / key loads issued before them
// is vmcnt(5), not a drain of the next molecule's staging
template <bool kMask>
__device__ __forceinline__ void stage_vp(const float* __restrict__ pv, int64_t ld,
                                         const float* __restrict__ P, int64_t b, float* lds, int h,
                                         int lane, int W) {
  const int64_t HD = (int64_t)kConvC * (kMask ? W : kFuseW);
  const float* pb = uniform_ptr(P + b * (kConvC * NT * NT)) + min(4 * lane, kConvC * NT * NT - 4);
#pragma unroll
  for (int k = 0; k < 5; ++k) {  // branch-free (selects): the wait counts stay exact
    const int piece = 5 * h + k;
    const int t = min(piece, kStV - 1) / 18;
    const float* vb;
    if (kMask)  // a lane past the end of the 12 W-float row re-reads the row's last float4
      vb = uniform_ptr(pv + (b * NT + t) * ld + HD) +
           min((min(piece, kStV - 1) % 18) * 256 + 4 * lane, (int)HD - 4);
    else
      vb = uniform_ptr(pv + (b * NT + t) * ld + HD + (min(piece, kStV - 1) % 18) * 256) + 4 * lane;
    const bool isv = piece < kStV;  // else the P piece (repeats write the same bytes)
    glds16(isv ? vb : pb, lds + (isv ? kOffV + piece * 256 : kOffP));
  }
}

template <bool kMask, int kV>
__global__ void __launch_bounds__(kFuseThreads, 3)  // one workgroup per CU
attn_conv_bwd_kernel(int64_t B, int64_t per_block, const float* __restrict__ pv, int64_t ld,
                     const float* __restrict__ x, int64_t ldx, float scale,
                     const float* __restrict__ P, const float* __restrict__ wgt,
                     const float* __restrict__ out, const float* __restrict__ g_out, float g_scale,
                     float* __restrict__ gpv, int64_t ldg, float* __restrict__ gk, int64_t ldgk,
                     uint32_t* __restrict__ gpv_amax, float* __restrict__ part,
                     uint32_t* __restrict__ gpv_rows, int dk) {
  constexpr int H = kConvC;
  const int W = kMask ? dk : kFuseW, Wo = W - 2;
  const int64_t HD = (int64_t)H * W;
  constexpr int kCD = kConvC * kConvH / 2;  // cube-gradient rows per thread
  __shared__ __attribute__((aligned(16))) float lds[kBwdLds];
  float* s_in = lds;
  const float* s_o = lds + kOffO;
  const float* s_v = lds + kOffV;   // [3][12 x W], row stride kStVRow
  const float* s_p = lds + kOffP;   // [12][9]
  const int tid = threadIdx.x, lane = tid & 63;
  const int h = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar branches
  const int lo = lane & 15, lk = lane >> 4;
  if (tid < 8) s_in[kConvC * kConvH * kConvLd + tid] = 0.f;
  for (int i = tid; i < kConvC * kConvH * (kConvLd - W); i += kFuseThreads)  // pad columns: finite
    s_in[(i / (kConvLd - W)) * kConvLd + W + i % (kConvLd - W)] = 0.f;
  f32x4_t acc[kConvNT];
#pragma unroll
  for (int j = 0; j < kConvNT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  int boff[kConvNT];
#pragma unroll
  for (int j = 0; j < kConvNT; ++j) {
    const int n = 16 * j + lo;
    boff[j] = n < 108 ? (n / 3) * kConvLd + n % 3 : (n == 108 ? -1 : -2);
  }
  // g_pre[o][x] (masked in place over the staged g_out rows at (A)); 0 outside [0, Wo), by
  // select on an always-in-range address (no branch around the LDS read)
  float* s_gp = lds + kOffG;
  auto gpre = [&](int o, int xx) -> float {
    const float v = s_gp[o * Wo + min(max(xx, 0), Wo - 1)];
    return (xx >= 0 && xx < Wo) ? v : 0.f;
  };
  float gmx = 0.f, pb = 0.f;
  // cube-gradient role; half is wave-uniform (W = 6 waves), so its weights are scalar loads.
  // kMask: the split is by W rounded up to whole waves (Wr <= 384), so half stays wave-uniform;
  // the lanes xp >= W of a wave compute on clamped addresses and store nothing, the waves past
  // 2 Wr threads (half >= 2) skip the role
  const int Wr = kMask ? (W + 63) & ~63 : W;
  const int xp = tid % Wr, half = __builtin_amdgcn_readfirstlane(tid / Wr);
  const int64_t b0 = (int64_t)blockIdx.x * per_block, b1 = min(B, b0 + per_block);
  if (b0 < b1) {
    stage_go<kMask>(g_out, out, b0, lds, h, lane, W);
    stage_vp<kMask>(pv, ld, P, b0, lds, h, lane, W);
  }
  for (int64_t b = b0; b < b1; ++b) {
    const bool next = b + 1 < b1;
    // (A) molecule b's staging landed (this wave's pieces; the barrier: everyone's); then
    // g_pre = g_out (out > 0) in place
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int e = tid; e < kConvO * Wo; e += kFuseThreads)
      s_gp[e] = s_o[e] > 0.f ? (g_scale == 1.f ? s_gp[e] : s_gp[e] * g_scale) : 0.f;
    // (B) the cube rows of head h
    {
      float p[NT][NT], v[NT][kV];
#pragma unroll
      for (int e = 0; e < NT * NT; ++e) p[e / NT][e % NT] = s_p[h * NT * NT + e];
      load_rows3<kMask>(s_v + (int64_t)h * W, (int64_t)kStVRow, lane, v, W);
      fold_att_lds<kMask>(p, v, s_in + h * NT * kConvLd, lane, W);
    }
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    // (C) weight / bias gradient
    if (kMask) {  // the steps at or past Wo (g_pre = 0 there: they add nothing) are not run
      const int ks1 = min(8 * h + 8, (Wo + 3) >> 2);
      for (int ks = 8 * h; ks < ks1; ++ks) {
        const int xx = 4 * ks + lk;
        const float av = lo < kConvO ? gpre(lo, xx) : 0.f;
#pragma unroll
        for (int j = 0; j < kConvNT; ++j) {
          const float bv = boff[j] >= 0 ? s_in[boff[j] + xx] : (boff[j] == -1 ? 1.f : 0.f);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
        }
      }
    } else {
#pragma unroll 2
      for (int ks = 8 * h; ks < 8 * h + 8; ++ks) {
        const int xx = 4 * ks + lk;
        const float av = lo < kConvO ? gpre(lo, xx) : 0.f;
#pragma unroll
        for (int j = 0; j < kConvNT; ++j) {
          const float bv = boff[j] >= 0 ? s_in[boff[j] + xx] : (boff[j] == -1 ? 1.f : 0.f);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
        }
      }
    }
    {  // bias of channel h: this molecule's row sum, then the running sum (short chains)
      float sb = 0.f;
#pragma unroll
      for (int i = 0; i < kV; ++i) sb += gpre(h, lane + 64 * i);
      pb += wave_sum(sb);
    }
    __builtin_amdgcn_sched_barrier(0);  // phases stay apart (registers)
    // (D) the cube's gradient in registers
    float acc_in[kCD];
    if (!kMask || half < 2) {
      int xpl = xp;  // laundered per molecule: the 36 row addresses are not hoisted out of the loop
      asm volatile("" : "+v"(xpl));
#pragma unroll
      for (int i = 0; i < kCD; ++i) acc_in[i] = 0.f;
      // the weights as SCALAR loads (constant address space: s_load, K$-resident) issued per
      // molecule; laundering the pointer keeps the compiler from hoisting all 648 of them out of
      // the molecule loop (SGPR spills).  A generic pointer here compiles to flat vector loads,
      // each batch drained by vmcnt(0) lgkmcnt(0) — 25 full memory latencies per molecule.
      const float* wh = wgt + half * kCD * 3;
      asm volatile("" : "+s"(wh));
      const __attribute__((address_space(4))) float* wc =
          (const __attribute__((address_space(4))) float*)wh;
      // g_pre rows one output channel at a time (3 values live, not 36)
#pragma unroll 2
      for (int o = 0; o < kConvO; ++o) {  // (o, dx) order as conv3_bwd2_kernel
        const auto* w = wc + o * (kConvC * kConvH * 3);
        float g[3];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) g[dx] = gpre(o, xpl - dx);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
          for (int cd = 0; cd < kCD; ++cd) acc_in[cd] = fmaf(w[cd * 3 + dx], g[dx], acc_in[cd]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every staged-row / cube read done
#pragma unroll
    for (int cd = 0; cd < kCD; ++cd)
      if (!kMask || (half < 2 && xp < W)) s_in[(half * kCD + cd) * kConvLd + xp] = acc_in[cd];
    float v[NT][kV], p[NT][NT];
#pragma unroll
    for (int e = 0; e < NT * NT; ++e) p[e / NT][e % NT] = s_p[h * NT * NT + e];
    load_rows3<kMask>(s_v + (int64_t)h * W, (int64_t)kStVRow, lane, v, W);
    if (next) stage_go<kMask>(g_out, out, b + 1, lds, h, lane, W);  // after the stores: registers
    // head h's query rows and the keys (plain loads: the compiler's wait at their first use
    // also covers the LDS-DMA pieces issued before it, so the next molecule's staging and these
    // loads share one memory latency)
    float q[NT][kV], k[NT][kV];
    load_rows3<kMask>(pv + b * NT * ld + (int64_t)h * W, ld, lane, q, W);
    load_rows3<kMask>(x + b * NT * ldx, ldx, lane, k, W);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // cube gradient stored; v / P read
    // unconditional (the last molecule re-stages its own v / P, already in registers): a fixed
    // count of DMA pieces per wave keeps the compiler's wait below at vmcnt(5)
    stage_vp<kMask>(pv, ld, P, next ? b + 1 : b, lds, h, lane, W);
    __builtin_amdgcn_sched_barrier(0);
    // (E) attention backward of head h (token_attn_fold_bwd_kernel's order)
    {
      float g[NT][kV];
      load_rows3<kMask>(s_in + h * NT * kConvLd, kConvLd, lane, g, W);
      float gs[NT][NT];
      fold_grad_scores(g, v, p, scale, gs);
      float rmx[NT];  // this wave's part of each token row's |max| (gpv_rows)
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        float* grow = gpv + (b * NT + c) * ldg + HD + (int64_t)h * W;
        rmx[c] = 0.f;
#pragma unroll
        for (int i = 0; i < kV; ++i) {
          float o = 0.f;
#pragma unroll
          for (int a = 0; a < NT; ++a) o = fmaf(p[a][c], g[a][i], o);
          if (col_ok<kMask, kV>(lane, i, W)) grow[lane + 64 * i] = o;
          rmx[c] = fmaxf(rmx[c], fabsf(o));
        }
      }
      // the keys' gradient partial of head h goes over head h's own cube rows (read above by
      // this wave only)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        float* grow = gpv + (b * NT + t) * ldg + (int64_t)h * W;
#pragma unroll
        for (int i = 0; i < kV; ++i) {
          float oq = 0.f, ok = 0.f;
#pragma unroll
          for (int c = 0; c < NT; ++c) {
            oq = fmaf(gs[t][c], k[c][i], oq);
            ok = fmaf(gs[c][t], q[c][i], ok);
          }
          if (col_ok<kMask, kV>(lane, i, W)) grow[lane + 64 * i] = oq;
          rmx[t] = fmaxf(rmx[t], fabsf(oq));
          if (col_ok<kMask, kV>(lane, i, W)) s_in[(h * NT + t) * kConvLd + lane + 64 * i] = ok;
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        gmx = fmaxf(gmx, rmx[t]);
        if (gpv_rows) {  // the twelve head waves' parts of the row: an order-free max
          const float m = wave_max(rmx[t]);
          if (lane == 0) atomicMax(gpv_rows + b * NT + t, __float_as_uint(m));
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int e = tid; e < NT * W; e += kFuseThreads) {  // g_k = sum over heads in head order
      const int t = e / W, c = e % W;
      float s = 0.f;
#pragma unroll
      for (int hh = 0; hh < H; ++hh) s += s_in[(hh * NT + t) * kConvLd + c];
      gk[(b * NT + t) * ldgk + c] = s;
    }
  }
  if (gpv_amax) {  // one unsigned atomicMax of the float bits per wave
    gmx = wave_max(gmx);
    if (lane == 0) atomicMax(gpv_amax, __float_as_uint(gmx));
  }
  // fixed-order reduction of the twelve waves' 12 x 109 weight-gradient tiles (rows o < 12)
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  float* red = lds;  // 12 x 12 x 112 floats <= the LDS array
  static_assert(kFuseWaves * kConvO * 112 <= kBwdLds, "reduction fits the LDS");
#pragma unroll
  for (int j = 0; j < kConvNT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * lk + r < kConvO) red[(h * kConvO + 4 * lk + r) * 112 + 16 * j + lo] = acc[j][r];
  __syncthreads();
  for (int i = tid; i < kConvO * 108; i += kFuseThreads) {
    const int o = i / 108, n = i % 108;
    float s = 0.f;
    for (int w = 0; w < kFuseWaves; ++w) s += red[(w * kConvO + o) * 112 + n];
    part[(int64_t)blockIdx.x * kConvPart + o * 108 + n] = s;
  }
  if (lane == 0) part[(int64_t)blockIdx.x * kConvPart + 2 * kConvWg + h] = pb;
}

}  // namespace
}  // namespace mvml

using namespace mvml;

static int64_t fused_blocks(int64_t B) { return std::min<int64_t>(B, 256); }  // 1 per CU

extern "C" int mvml_attn_conv_fwd(int64_t B, int H, int dk, const float* pv, int64_t ld,
                                  const float* x, int64_t ldx, float scale, const float* weight,
                                  const float* bias, float* P, float* out, double drop_p,
                                  int64_t drop_seed, void* stream) {
  clear_error();
  MVML_REQUIRE(B >= 0 && H == kConvC && fuse_dk_ok(dk) && ld >= 2 * (int64_t)H * dk && ldx >= dk,
               "attn_conv_fwd: H must be %d, " MVML_DK_SET ", ld >= 2*H*dk, ldx >= dk", kConvC);
  MVML_REQUIRE(drop_p >= 0.0 && drop_p < 1.0, "attn_conv_fwd: dropout p must be in [0, 1)");
  if (B == 0) return MVML_OK;
  const int64_t nblk = fused_blocks(B), per = ceil_div(B, nblk);
  return by_width(dk, [&](auto mask, auto kv) {
    attn_conv_fwd_kernel<mask.value, kv.value><<<(unsigned)ceil_div(B, per), kFuseThreads, 0, as_stream(stream)>>>(
        B, per, pv, ld, x, ldx, scale, weight, bias, P, out, drop_p > 0.0 ? dropout_threshold(drop_p) : 0u,
        dropout_scale(drop_p), (uint64_t)drop_seed, dk);
    return check_launch("attn_conv_fwd_kernel");
  });
}

extern "C" size_t mvml_attn_conv_bwd_workspace_size(int64_t B) {
  return carve_size((size_t)fused_blocks(B > 0 ? B : 1) * kConvPart * sizeof(float));
}

extern "C" int mvml_attn_conv_bwd(int64_t B, int H, int dk, const float* pv, int64_t ld,
                                  const float* x, int64_t ldx, float scale, const float* P,
                                  const float* weight, const float* out, const float* g_out,
                                  float g_scale, float* g_pv, int64_t ldg, float* g_k, int64_t ldgk,
                                  uint32_t* g_pv_amax, uint32_t* g_pv_rows, float* g_weight,
                                  float* g_bias, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  clear_error();
  MVML_REQUIRE(B >= 0 && H == kConvC && fuse_dk_ok(dk) && ld >= 2 * (int64_t)H * dk &&
                   ldx >= dk && ldg >= 2 * (int64_t)H * dk && ldgk >= dk,
               "attn_conv_bwd: H must be %d, " MVML_DK_SET ", ld / ldg >= 2*H*dk, ldx / ldgk >= dk",
               kConvC);
  // the staging reads pv's v columns, P, out and g_out as 16-byte pieces
  MVML_REQUIRE(ld % 4 == 0 && aligned16(pv) && aligned16(P) && aligned16(out) && aligned16(g_out),
               "attn_conv_bwd: pv, P, out and g_out must be 16-byte aligned and ld a multiple of 4");
  if (B == 0) return MVML_OK;
  if (!workspace || workspace_bytes < mvml_attn_conv_bwd_workspace_size(B)) {
    set_error("attn_conv_bwd: workspace of mvml_attn_conv_bwd_workspace_size bytes required");
    return MVML_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int64_t nblk = fused_blocks(B), per = ceil_div(B, nblk);
  const int64_t used = ceil_div(B, per);
  float* part = static_cast<float*>(workspace);
  const int rc = by_width(dk, [&](auto mask, auto kv) {
    attn_conv_bwd_kernel<mask.value, kv.value><<<(unsigned)used, kFuseThreads, 0, st>>>(
        B, per, pv, ld, x, ldx, scale, P, weight, out, g_out, g_scale, g_pv, ldg, g_k, ldgk, g_pv_amax,
        part, g_pv_rows, dk);
    return check_launch("attn_conv_bwd_kernel");
  });
  if (rc) return rc;
  return sum_conv_partials((int)used, part, g_weight, g_bias, st);
}
