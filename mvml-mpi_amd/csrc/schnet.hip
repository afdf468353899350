// SchNet's continuous-filter convolution (dgl 0.9.1 CFConv, dgllife 0.3.0 SchNetGNN; restated, parity
// with dgllife unpinned) without the [E, K] radial-basis expansion in memory.  For an edge s = (u -> v)
// with distance d_s, centres mu [K], gamma = 1 / gap and ssp(x) = softplus(x) - ln 2:
//
//   rbf_s[k] = exp(-gamma (d_s - mu_k)^2)           (a function of ONE float per edge: never stored)
//   s1_s = ssp(rbf_s W_1^T + b_1)   he_s = ssp(s1_s W_2^T + b_2)   a_v = sum_{u -> v} hv[u] * he_s
//
// schnet_filter_fwd_kernel: a workgroup of four waves owns kSnTile = 128 consecutive in-CSR slots and
// all H <= 128 columns; a wave owns 32 rows as two 16-row MFMA blocks.  Product 1's A operand is never
// loaded: per 32-wide k-step a lane computes the eight values exp(-gamma (d - mu_k)^2) of its row and
// k group (fragment layout: row = lane & 15, k = 32 ks + 8 (lane >> 4) + j) from the row's one distance
// and the centres (staged in LDS once, padded centres give exactly 0), scales them by the fixed 2^14
// (rbf lies in (0, 1]: no row maximum) and splits them into two fp16 planes in registers
// (gemm_common.h split2h8).  W_1 and W_2 are split once per weight value into fragment-ordered images
// (schnet_split_kernel: [k-step][16-column block][{h, l}][64 lanes] x 16 B); a panel = one k-step of up
// to four column blocks is one contiguous run that the four waves stream from L2 through a two-slot
// LDS ring, one barrier per panel (as nnconv.hip; 16 KiB whatever K and H are).  Per panel, row block
// and column block: 3 v_mfma_f32_16x16x32_f16 (l h, h l, h h).  After the first ssp the wave's s1 block
// goes through a wave-private LDS window, 16 rows at a time, from accumulator layout (rows 4 lg + r,
// column lr) to A-fragment layout, is split per row with the row's own scale and multiplied by W_2's
// image without leaving the CU.  s1 and he are stored; ssp' is taken from the OUTPUT,
// sigmoid(pre) = 1 - 0.5 exp(-ssp(pre)), so no pre-activation and nothing of width K is stored.
//
// schnet_filter_bwd_kernel: the same tile.  dhe_s = dA[dst s] * hv[src s] is formed on load, directly
// in A-fragment layout (eight consecutive columns per lane: three 2 x 16-B loads), dpre2 = dhe ssp'(he)
// is stored from there and split per row; ds1 = dpre2 W_2 runs on W_2's transposed image, and
// dpre1 = ds1 ssp'(s1) leaves from the accumulators.  dhe never reaches memory.
//
// schnet_dw1_kernel: dW_1[j, k] = sum_s dpre1[s, j] rbf_s[k] contracts over the slots, so dpre1's rows
// are the MFMA A operand as they lie (v_mfma_f32_16x16x4f32: A lanes run along 16 contiguous j) and
// the B operand, rbf, is generated: lane (lr, lg) computes exp(-gamma (d_{4 q + lg} - mu_{16 cb + lr})^2),
// one exp per MFMA step and (slot, centre).  Grid (slot range, 64 centres): a wave owns 16 centres and
// all H / 16 row blocks; the slot ranges' partials are summed in fixed order (colsum_final_launch),
// onto dW_1 when accumulating.  fp32 MFMA, not split-fp16: the split form needs dpre1 transposed
// through LDS and re-split per chunk, and the product is small beside the exps.
//
// cfconv_agg_kernel: out[v] = sum_i X[xidx[w_i]] * Wt[w_i] over v's list (w_i = widx ? widx[i] : i), i
// ascending from 0, one fma (one rounding) per entry.  One wave per atom, lanes on the float4 columns
// (H <= 64: 16 lanes per atom, four atoms per wave, as gcn_agg.hip and dmpnn.hip); long lists are
// walked in chunks of the lane group, so a hub needs no LDS.  Forward: v's in-slot range, xidx =
// in_src, Wt = he in order.  Gradient of hv: v's out-edges (widx = out_inslot), X = dA gathered at the
// slot's destination (xidx = slot_dst), Wt = he at that slot.  An empty list gives exact zeros.
//
// No float atomics anywhere: bitwise repeatable, and a slot's or an atom's bits do not depend on the
// batch around it.
#include "gemm_common.h"
#include "wave_ops.h"

namespace mvml {
namespace {

constexpr int kSnTile = 128;    // slots per workgroup: 4 waves x 2 MFMA row blocks of 16
constexpr int kSnPanel = 512;   // uint4 per ring slot: 4 column blocks x {h, l} x 64 lanes
constexpr int kSnMaxK = 512;
constexpr int kSnMaxH = 128;
constexpr int kSnRbfShift = 14; // rbf in (0, 1] scaled by 2^14: below fp16's 65504, the low plane normal
constexpr int kSnWgE = 32;      // slots per staged chunk of the W_1 gradient
constexpr int kSnWgP = kSnMaxH + 16;  // its LDS row pitch (pitch % 64 == 16, nnconv.hip nn_pitch)
constexpr int kSnMaxSplits = 128;
constexpr float kLn2 = 0.69314718055994531f;

// softplus(x) - ln 2 with torch's beta 1 and threshold 20, and its derivative from its OUTPUT
__device__ __forceinline__ float ssp(float x) { return (x > 20.f ? x : log1pf(expf(x))) - kLn2; }
__device__ __forceinline__ float ssp_grad(float y) { return 1.f - 0.5f * expf(-y); }
__device__ __forceinline__ float rbf(float d, float mu, float gamma) {
  const float t = d - mu;
  return expf(-gamma * (t * t));
}

__host__ __device__ inline int sn_ks(int K) { return (K + 31) / 32; }
inline size_t img1_vec(int H, int K) { return (size_t)sn_ks(K) * (H / 16) * 128; }
inline size_t img2_vec(int H) { return (size_t)sn_ks(H) * (H / 16) * 128; }
struct SnImage {  // [256 B: bits of max |W_1|, max |W_2|][W_1][W_2][W_2 transposed]
  const uint32_t* amax;
  const uint4 *w1, *w2, *w2t;
  SnImage(const void* p, int H, int K)
      : amax(static_cast<const uint32_t*>(p)), w1(reinterpret_cast<const uint4*>(static_cast<const char*>(p) + 256)),
        w2(w1 + img1_vec(H, K)), w2t(w2 + img2_vec(H)) {}
};

// One thread per (image, k-step, column block, lane), eight k values each: B[k][n] =
//   W_1[n K + k] (k < K, else 0) | W_2[n H + k] | W_2[k H + n]
__global__ void __launch_bounds__(256)
schnet_split_kernel(int H, int K, const float* __restrict__ W1, const float* __restrict__ W2,
                    const uint32_t* __restrict__ amax, uint4* __restrict__ img) {
  const int NT = H / 16;
  const int64_t n1 = (int64_t)sn_ks(K) * NT * 64, n2 = (int64_t)sn_ks(H) * NT * 64;
  int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n1 + 2 * n2) return;
  const int which = idx < n1 ? 0 : idx < n1 + n2 ? 1 : 2;
  uint4* base = img + (which == 0 ? 0 : which == 1 ? 2 * n1 : 2 * (n1 + n2));
  idx -= which == 0 ? 0 : which == 1 ? n1 : n1 + n2;
  const int lane = (int)(idx & 63);
  const int64_t pn = idx >> 6;  // ks NT + nt
  const int nt = (int)(pn % NT), ks = (int)(pn / NT);
  const int n = nt * 16 + (lane & 15), k0 = ks * 32 + (lane >> 4) * 8;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    v[j] = which == 0 ? (k < K ? W1[(int64_t)n * K + k] : 0.f)
                      : (k < H ? (which == 1 ? W2[(int64_t)n * H + k] : W2[(int64_t)k * H + n]) : 0.f);
  }
  bf16x8 h, l;
  split2h8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]),
           pow2f(amax_shift(amax[which ? 1 : 0])), h, l);
  uint4* dst = base + pn * 128 + lane;
  dst[0] = __builtin_bit_cast(uint4, h);
  dst[64] = __builtin_bit_cast(uint4, l);
}

// acc[rt][nt] += A(ks) B(ks, nt) over the nks k-steps of an image, streamed panel by panel (k-step, four
// column blocks) through the two-slot ring.  getA(ks, ah, al) yields the wave's two row blocks' planes
// of k-step ks.  KSU > 0: the k loop is unrolled (A held in registers, indexed at compile time); 0: a
// run-time loop (A generated).  Every wave of the workgroup calls it; it ends on a barrier.
template <int NTB, int KSU, typename GetA>
__device__ __forceinline__ void sn_product(int nks, int NT, const uint4* __restrict__ img, uint4* ring, int tid,
                                           int lane, GetA&& getA, f32x4 (&acc)[2][NTB]) {
  constexpr int NGB = (NTB + 3) / 4;
  u32x4 pre[2];
  int pcnt = 0;
  auto fetch = [&](int ks, int ng) __attribute__((always_inline)) {
    pcnt = min(4, NT - 4 * ng) * 128;
    const uint4* p = img + ((int64_t)ks * NT + 4 * ng) * 128;
#pragma unroll
    for (int l = 0; l < 2; ++l)
      if (tid + 256 * l < pcnt) pre[l] = __builtin_bit_cast(u32x4, p[tid + 256 * l]);
  };
  auto park = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int l = 0; l < 2; ++l)
      if (tid + 256 * l < pcnt) ring[slot * kSnPanel + tid + 256 * l] = __builtin_bit_cast(uint4, pre[l]);
  };
  fetch(0, 0);
  park(0);
  __syncthreads();
  int buf = 0;
  auto step = [&](int ks) __attribute__((always_inline)) {
    f16x8 ah[2], al[2];
    getA(ks, ah, al);
#pragma unroll
    for (int ng = 0; ng < NGB; ++ng) {
      if (4 * ng < NT) {  // (uniform over the workgroup)
        const bool wrap = 4 * (ng + 1) >= NT, last = wrap && ks == nks - 1;
        if (!last) fetch(wrap ? ks + 1 : ks, wrap ? 0 : ng + 1);
        const uint4* pb = ring + buf * kSnPanel;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (4 * ng + j < NTB && 4 * ng + j < NT) {
            const f16x8 bh = __builtin_bit_cast(f16x8, pb[(2 * j) * 64 + lane]);
            const f16x8 bl = __builtin_bit_cast(f16x8, pb[(2 * j + 1) * 64 + lane]);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
              f32x4 c = acc[rt][(4 * ng + j) % NTB];
              c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rt], bh, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt], bl, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt], bh, c, 0, 0, 0);
              acc[rt][(4 * ng + j) % NTB] = c;
            }
          }
        }
        if (!last) park(buf ^ 1);
        __syncthreads();
        buf ^= 1;
      }
    }
  };
  if constexpr (KSU > 0) {
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks)
      if (ks < nks) step(ks);
  } else {
    for (int ks = 0; ks < nks; ++ks) step(ks);
  }
}

struct SnFwdArgs {
  int64_t E;
  const float* d;  // [E] at stride ldd, slot order
  int64_t ldd;
  const float* centers;
  int K;
  float gamma;
  int H;
  const uint32_t* amax;
  const uint4 *img1, *img2;
  const float *b1, *b2;
  float* s1;
  int64_t lds1;
  float* he;
  int64_t ldhe;
};

// NTB: the 16-column blocks the instance holds accumulators for (H <= 16 NTB).
template <int NTB>
__global__ void __launch_bounds__(256) schnet_filter_fwd_kernel(SnFwdArgs a) {
  constexpr int P = NTB * 16 + 4;      // window row pitch (P % 16 == 4: the four row groups hit distinct banks)
  constexpr int KSU = NTB >= 2 ? NTB / 2 : 1;  // k-steps of product 2
  __shared__ uint4 ring[2 * kSnPanel];
  __shared__ float cs[kSnMaxK];
  __shared__ float win[4][16 * P];     // a wave's 16-row window; column H of a row: its scale shift
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * kSnTile + wave * 32;
  const int H = a.H, NT = H / 16, K = a.K;
  for (int i = tid; i < sn_ks(K) * 32; i += 256) cs[i] = i < K ? a.centers[i] : 0.f;
  float dr[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t s = e0 + rt * 16 + lr;
    dr[rt] = s < a.E ? a.d[s * a.ldd] : 0.f;
  }
  __syncthreads();
  f32x4 acc[2][NTB];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nt = 0; nt < NTB; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float gamma = a.gamma;
  auto gen = [&](int ks, f16x8 (&ah)[2], f16x8 (&al)[2]) __attribute__((always_inline)) {
    const int k0 = ks * 32 + lg * 8;
    const float4 c0 = ld4(cs + k0), c1 = ld4(cs + k0 + 4);
    const float mu[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = k0 + j < K ? rbf(dr[rt], mu[j], gamma) : 0.f;  // padded centres: exactly 0
      bf16x8 hh, ll;
      split2h8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), pow2f(kSnRbfShift), hh, ll);
      ah[rt] = __builtin_bit_cast(f16x8, hh);
      al[rt] = __builtin_bit_cast(f16x8, ll);
    }
  };
  sn_product<NTB, 0>(sn_ks(K), NT, a.img1, ring, tid, lane, gen, acc);

  // s1 = ssp(. + b_1): stored, then through the wave's window into A-fragment layout, split per row
  const float u1 = pow2f(-kSnRbfShift - amax_shift(a.amax[0]));
  f16x8 sh[2][KSU], sl[2][KSU];
  int rsh[2][4];
  float* w = win[wave];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < NTB; ++nt) {
      if (nt < NT) {
        const int col = 16 * nt + lr;
        const float b = a.b1[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = ssp(__fmaf_rn(acc[rt][nt][r], u1, b));
          m[r] = fmaxf(m[r], fabsf(v));
          const int64_t s = e0 + rt * 16 + 4 * lg + r;
          if (s < a.E) a.s1[s * a.lds1 + col] = v;
          w[(4 * lg + r) * P + col] = v;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o, 64));
      rsh[rt][r] = amax_shift(__float_as_uint(m[r]));
      if (lr == 0) w[(4 * lg + r) * P + H] = __int_as_float(rsh[rt][r]);
    }
    wave_sync_lds();
    const float sc = pow2f(__float_as_int(w[lr * P + H]));
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) {
      const int k0 = ks * 32 + lg * 8;
      const bool ok = k0 < H;  // (H % 16 == 0: a group of eight is whole or absent)
      const float4 lo = ok ? ld4(w + lr * P + k0) : f4(0.f), hi = ok ? ld4(w + lr * P + k0 + 4) : f4(0.f);
      bf16x8 hh, ll;
      split2h8(lo, hi, sc, hh, ll);
      sh[rt][ks] = __builtin_bit_cast(f16x8, hh);
      sl[rt][ks] = __builtin_bit_cast(f16x8, ll);
    }
    wave_sync_lds();  // the reads are done before the next row block's writes
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nt = 0; nt < NTB; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto held = [&](int ks, f16x8 (&ah)[2], f16x8 (&al)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      ah[rt] = sh[rt][ks];
      al[rt] = sl[rt][ks];
    }
  };
  sn_product<NTB, KSU>(sn_ks(H), NT, a.img2, ring, tid, lane, held, acc);
  const float u2 = pow2f(-amax_shift(a.amax[1]));
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t s = e0 + rt * 16 + 4 * lg + r;
      if (s >= a.E) continue;
      const float usc = pow2f(-rsh[rt][r]) * u2;
#pragma unroll
      for (int nt = 0; nt < NTB; ++nt)
        if (nt < NT) a.he[s * a.ldhe + 16 * nt + lr] = ssp(__fmaf_rn(acc[rt][nt][r], usc, a.b2[16 * nt + lr]));
    }
}

struct SnBwdArgs {
  int64_t E;
  const int32_t *src, *dst;  // in_src, slot_dst
  const float* dA;
  int64_t lda;
  const float* hv;
  int64_t ldh;
  const float* s1;
  int64_t lds1;
  const float* he;
  int64_t ldhe;
  int H;
  const uint32_t* amax;
  const uint4* img2t;
  float* dpre2;
  int64_t ld2;
  float* dpre1;
  int64_t ld1;
};

__device__ __forceinline__ float4 dpre_of(float4 g, float4 h, float4 y) {
  return make_float4(__fmul_rn(__fmul_rn(g.x, h.x), ssp_grad(y.x)), __fmul_rn(__fmul_rn(g.y, h.y), ssp_grad(y.y)),
                     __fmul_rn(__fmul_rn(g.z, h.z), ssp_grad(y.z)), __fmul_rn(__fmul_rn(g.w, h.w), ssp_grad(y.w)));
}
__device__ __forceinline__ float amax_of(float m, float4 v) {
  return fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}

template <int NTB>
__global__ void __launch_bounds__(256) schnet_filter_bwd_kernel(SnBwdArgs a) {
  constexpr int KSU = NTB >= 2 ? NTB / 2 : 1;
  __shared__ uint4 ring[2 * kSnPanel];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * kSnTile + wave * 32;
  const int H = a.H, NT = H / 16;
  f16x8 ah[2][KSU], al[2][KSU];
  int rsh[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t s = e0 + rt * 16 + lr;
    const bool live = s < a.E;
    const float* gr = live ? a.dA + (int64_t)a.dst[s] * a.lda : nullptr;
    const float* hr = live ? a.hv + (int64_t)a.src[s] * a.ldh : nullptr;
    float4 lo[KSU], hi[KSU];
    float m = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) {
      const int k0 = ks * 32 + lg * 8;
      lo[ks] = hi[ks] = f4(0.f);
      if (live && k0 < H) {  // dpre2 = (dA[dst] * hv[src]) ssp'(he), formed and stored in fragment layout
        const float* yr = a.he + s * a.ldhe + k0;
        lo[ks] = dpre_of(ld4(gr + k0), ld4(hr + k0), ld4(yr));
        hi[ks] = dpre_of(ld4(gr + k0 + 4), ld4(hr + k0 + 4), ld4(yr + 4));
        st4(a.dpre2 + s * a.ld2 + k0, lo[ks]);
        st4(a.dpre2 + s * a.ld2 + k0 + 4, hi[ks]);
        m = amax_of(amax_of(m, lo[ks]), hi[ks]);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));  // the row's four lane groups
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    rsh[rt] = amax_shift(__float_as_uint(m));
    const float sc = pow2f(rsh[rt]);
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) {
      bf16x8 hh, ll;
      split2h8(lo[ks], hi[ks], sc, hh, ll);
      ah[rt][ks] = __builtin_bit_cast(f16x8, hh);
      al[rt][ks] = __builtin_bit_cast(f16x8, ll);
    }
  }
  f32x4 acc[2][NTB];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nt = 0; nt < NTB; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto held = [&](int ks, f16x8 (&xh)[2], f16x8 (&xl)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      xh[rt] = ah[rt][ks];
      xl[rt] = al[rt][ks];
    }
  };
  sn_product<NTB, KSU>(sn_ks(H), NT, a.img2t, ring, tid, lane, held, acc);
  const float u2 = pow2f(-amax_shift(a.amax[1]));
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float usc = pow2f(-__shfl(rsh[rt], 4 * lg + r, 64)) * u2;  // (every lane takes part)
      const int64_t s = e0 + rt * 16 + 4 * lg + r;
      if (s >= a.E) continue;
#pragma unroll
      for (int nt = 0; nt < NTB; ++nt)
        if (nt < NT) {
          const int col = 16 * nt + lr;
          a.dpre1[s * a.ld1 + col] = __fmul_rn(acc[rt][nt][r] * usc, ssp_grad(a.s1[s * a.lds1 + col]));
        }
    }
}

// Partial dW_1 over the slot range blockIdx.x, centres 64 blockIdx.y ..: part[x][j K + k].
__global__ void __launch_bounds__(256)
schnet_dw1_kernel(int64_t E, int64_t per, const float* __restrict__ d, int64_t ldd, const float* __restrict__ centers,
                  int K, float gamma, const float* __restrict__ g, int64_t ldg, int H, float* __restrict__ part) {
  __shared__ float gs[kSnWgE * kSnWgP];  // dpre1 rows
  __shared__ float ds[kSnWgE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int MT = H / 16, q4 = H / 4;
  const int k = (blockIdx.y * 4 + wave) * 16 + lr;
  const bool wave_live = (blockIdx.y * 4 + wave) * 16 < K;  // (uniform over the wave)
  const float mu = k < K ? centers[k] : 0.f;
  const int64_t e_beg = (int64_t)blockIdx.x * per, e_end = min(E, e_beg + per);
  f32x4 acc[8];
#pragma unroll
  for (int mt = 0; mt < 8; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t c0 = e_beg; c0 < e_end; c0 += kSnWgE) {
    __syncthreads();  // the previous chunk's reads are done
    for (int idx = tid; idx < kSnWgE * q4; idx += 256) {
      const int r = idx / q4, c = 4 * (idx - r * q4);
      const int64_t s = c0 + r;
      st4(gs + r * kSnWgP + c, s < e_end ? ld4(g + s * ldg + c) : f4(0.f));
    }
    if (tid < kSnWgE) ds[tid] = c0 + tid < e_end ? d[(c0 + tid) * ldd] : 0.f;
    __syncthreads();
    if (wave_live) {
#pragma unroll 2
      for (int q = 0; q < kSnWgE / 4; ++q) {
        const int e = 4 * q + lg;  // A: row j = 16 mt + lr, k = slot e; B: column = centre k, k = slot e
        const float bv = k < K ? rbf(ds[e], mu, gamma) : 0.f;  // (slots past the range: their dpre1 rows are 0)
#pragma unroll
        for (int mt = 0; mt < 8; ++mt)
          if (mt < MT) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gs[e * kSnWgP + 16 * mt + lr], bv, acc[mt], 0, 0, 0);
      }
    }
  }
  if (k >= K) return;
  float* pp = part + (int64_t)blockIdx.x * H * K;
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
    if (mt < MT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pp[(int64_t)(16 * mt + 4 * lg + r) * K + k] = acc[mt][r];
    }
}

template <int LW>
__device__ __forceinline__ int groups_max(int x) {  // over a wave's lane groups, x uniform in each
  if (LW < 64) {
    x = max(x, __shfl_xor(x, 16, 64));
    x = max(x, __shfl_xor(x, 32, 64));
  }
  return x;
}
__device__ __forceinline__ float4 fma4_rn(float4 x, float4 w, float4 c) {
  return make_float4(__fmaf_rn(x.x, w.x, c.x), __fmaf_rn(x.y, w.y, c.y), __fmaf_rn(x.z, w.z, c.z),
                     __fmaf_rn(x.w, w.w, c.w));
}

struct CfAggArgs {
  int64_t N;
  const int32_t *rowptr, *widx, *xidx;
  const float* X;
  int64_t ldx;
  const float* Wt;
  int64_t ldw;
  int H;
  float* out;
  int64_t ldo;
};

// LW lanes per atom, U list entries in flight.
template <int LW, int U>
__global__ void __launch_bounds__(256) cfconv_agg_kernel(CfAggArgs a) {
  const int lane = threadIdx.x & 63, sl = lane & (LW - 1), g0 = lane & ~(LW - 1);
  const int64_t v = (xcd_block(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)) * (64 / LW) + lane / LW;
  const bool row = v < a.N;
  const int b = row ? a.rowptr[v] : 0, n = row ? a.rowptr[v + 1] - b : 0;
  const int mn = groups_max<LW>(n);
  const int q = a.H / 4;
  for (int c0 = 0; c0 < q; c0 += LW) {  // (uniform; H <= 128: one pass)
    const bool ok = row && c0 + sl < q;
    const int c = 4 * (c0 + sl);
    float4 Q = f4(0.f);
    for (int base = 0; base < mn; base += LW) {  // more entries than lanes (hubs): more chunks
      const int cnt = max(0, min(LW, n - base));
      int w_l = 0, x_l = 0;
      if (sl < cnt) {
        w_l = a.widx ? a.widx[b + base + sl] : b + base + sl;
        x_l = a.xidx[w_l];
      }
      const int mcnt = groups_max<LW>(cnt);
      for (int j0 = 0; j0 < mcnt; j0 += U) {
        float4 x[U], w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = g0 + min(j0 + u, LW - 1);
          const int wi = __shfl(w_l, e, 64), xi = __shfl(x_l, e, 64);
          const bool live = ok && j0 + u < cnt;
          x[u] = live ? ld4(a.X + (int64_t)xi * a.ldx + c) : f4(0.f);
          w[u] = live ? ld4(a.Wt + (int64_t)wi * a.ldw + c) : f4(0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (ok && j0 + u < cnt) Q = fma4_rn(x[u], w[u], Q);  // list order, one rounding per entry
      }
    }
    if (ok) st4(a.out + v * a.ldo + c, Q);
  }
}

__global__ void __launch_bounds__(256) ssp_fwd_kernel(int64_t n, const float* x, float* y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = ssp(x[i]);
}
__global__ void __launch_bounds__(256)
ssp_bwd_kernel(int64_t n, const float* y, const float* gy, float* gx) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    gx[i] = __fmul_rn(gy[i], ssp_grad(y[i]));
}

int check_schnet(const char* who, int H, int K) {
  MVML_REQUIRE(H >= 16 && H <= kSnMaxH && H % 16 == 0, "%s: the filter width H must be a multiple of 16 in [16, %d] (got %d)",
               who, kSnMaxH, H);
  MVML_REQUIRE(K >= 1 && K <= kSnMaxK, "%s: 1 to %d radial-basis centres K (got %d)", who, kSnMaxK, K);
  return MVML_OK;
}
bool edges_ok(int64_t E) { return E >= 0 && E < (int64_t(1) << 31) - kSnTile; }
bool gamma_ok(float g) { return g > 0.f && g <= 3.0e38f; }

int dw1_splits(int64_t E) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(E, 4 * kSnWgE), kSnMaxSplits));
}

template <typename Fn>
int by_width(int H, Fn&& fn) {  // the instance that holds H's column blocks
  return H <= 32 ? fn(std::integral_constant<int, 2>{}) : H <= 64 ? fn(std::integral_constant<int, 4>{})
                                                                   : fn(std::integral_constant<int, 8>{});
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" size_t mvml_schnet_image_bytes(int H, int K) {
  if (H < 16 || H > kSnMaxH || H % 16 || K < 1 || K > kSnMaxK) return 0;
  return 256 + 16 * (img1_vec(H, K) + 2 * img2_vec(H));
}

extern "C" int mvml_schnet_split_w(int H, int K, const float* W1, const float* W2, void* image, void* stream) {
  clear_error();
  if (int rc = check_schnet("schnet_split_w", H, K)) return rc;
  MVML_REQUIRE(W1 != nullptr && W2 != nullptr && image != nullptr && aligned16(image),
               "schnet_split_w: W1, W2 and a 16-byte aligned image are required");
  const hipStream_t st = as_stream(stream);
  uint32_t* amax = static_cast<uint32_t*>(image);
  if (int rc = absmax_launch(H, K, W1, K, amax, false, st)) return rc;
  if (int rc = absmax_launch(H, H, W2, H, amax + 1, false, st)) return rc;
  SnImage im(image, H, K);
  const int64_t n = (int64_t)(img1_vec(H, K) + 2 * img2_vec(H)) / 2;
  schnet_split_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(H, K, W1, W2, im.amax, const_cast<uint4*>(im.w1));
  return check_launch("schnet_split_kernel");
}

extern "C" int mvml_schnet_filter_fwd(int64_t num_edges, const float* d, int64_t ldd, const float* centers, int K,
                                      float gamma, int H, const void* image, const float* b1, const float* b2,
                                      float* s1, int64_t lds1, float* he, int64_t ldhe, void* stream) {
  clear_error();
  if (int rc = check_schnet("schnet_filter_fwd", H, K)) return rc;
  MVML_REQUIRE(edges_ok(num_edges) && gamma_ok(gamma), "schnet_filter_fwd: bad num_edges %lld or gamma %g",
               (long long)num_edges, (double)gamma);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(d != nullptr && ldd >= 1 && centers != nullptr && image != nullptr && aligned16(image) && b1 != nullptr &&
                   b2 != nullptr,
               "schnet_filter_fwd: d (stride >= 1), centers, a 16-byte aligned image, b1 and b2 are required");
  MVML_REQUIRE(row_ok(s1, lds1, H) && row_ok(he, ldhe, H),
               "schnet_filter_fwd: s1 and he must be 16-byte aligned with pitches >= H that are multiples of 4");
  SnImage im(image, H, K);
  const SnFwdArgs a{num_edges, d, ldd, centers, K, gamma, H, im.amax, im.w1, im.w2, b1, b2, s1, lds1, he, ldhe};
  const unsigned grid = (unsigned)ceil_div(num_edges, kSnTile);
  const hipStream_t st = as_stream(stream);
  by_width(H, [&](auto n) {
    schnet_filter_fwd_kernel<decltype(n)::value><<<grid, 256, 0, st>>>(a);
    return MVML_OK;
  });
  return check_launch("schnet_filter_fwd_kernel");
}

extern "C" int mvml_schnet_filter_bwd(int64_t num_edges, const int32_t* in_src, const int32_t* slot_dst, const float* dA,
                                      int64_t lda, const float* hv, int64_t ldh, const float* s1, int64_t lds1,
                                      const float* he, int64_t ldhe, int H, int K, const void* image, float* dpre2,
                                      int64_t ld2, float* dpre1, int64_t ld1, void* stream) {
  clear_error();
  if (int rc = check_schnet("schnet_filter_bwd", H, K)) return rc;
  MVML_REQUIRE(edges_ok(num_edges), "schnet_filter_bwd: bad num_edges %lld", (long long)num_edges);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(in_src != nullptr && slot_dst != nullptr && image != nullptr && aligned16(image),
               "schnet_filter_bwd: in_src, slot_dst and a 16-byte aligned image are required");
  MVML_REQUIRE(row_ok(dA, lda, H) && row_ok(hv, ldh, H) && row_ok(s1, lds1, H) && row_ok(he, ldhe, H) &&
                   row_ok(dpre2, ld2, H) && row_ok(dpre1, ld1, H),
               "schnet_filter_bwd: dA, hv, s1, he, dpre2 and dpre1 must be 16-byte aligned with pitches >= H that are "
               "multiples of 4");
  SnImage im(image, H, K);
  const SnBwdArgs a{num_edges, in_src, slot_dst, dA, lda, hv, ldh, s1, lds1, he, ldhe, H, im.amax, im.w2t, dpre2, ld2,
                    dpre1, ld1};
  const unsigned grid = (unsigned)ceil_div(num_edges, kSnTile);
  const hipStream_t st = as_stream(stream);
  by_width(H, [&](auto n) {
    schnet_filter_bwd_kernel<decltype(n)::value><<<grid, 256, 0, st>>>(a);
    return MVML_OK;
  });
  return check_launch("schnet_filter_bwd_kernel");
}

extern "C" size_t mvml_schnet_dw1_workspace_size(int64_t num_edges, int H, int K) {
  if (num_edges < 0 || H <= 0 || K <= 0) return 0;
  return carve_size((size_t)dw1_splits(num_edges) * H * K * 4) + 256;
}

extern "C" int mvml_schnet_dw1(int64_t num_edges, const float* d, int64_t ldd, const float* centers, int K, float gamma,
                               const float* dpre1, int64_t ld1, int H, int accumulate, float* dW1, void* workspace,
                               size_t workspace_bytes, void* stream) {
  clear_error();
  if (int rc = check_schnet("schnet_dw1", H, K)) return rc;
  MVML_REQUIRE(edges_ok(num_edges) && gamma_ok(gamma), "schnet_dw1: bad num_edges %lld or gamma %g", (long long)num_edges,
               (double)gamma);
  MVML_REQUIRE(dW1 != nullptr, "schnet_dw1: dW1 is required");
  const int64_t n = (int64_t)H * K;
  if (num_edges == 0) return accumulate ? MVML_OK : mvml_fill_zero(dW1, 1, n * 4, n * 4, stream);
  MVML_REQUIRE(d != nullptr && ldd >= 1 && centers != nullptr && row_ok(dpre1, ld1, H),
               "schnet_dw1: d (stride >= 1) and centers are required; dpre1 must be 16-byte aligned with a pitch >= H "
               "that is a multiple of 4");
  const size_t need = mvml_schnet_dw1_workspace_size(num_edges, H, K);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("schnet_dw1: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  const int S = dw1_splits(num_edges);
  const int64_t per = ceil_div(ceil_div(num_edges, kSnWgE), S) * kSnWgE;
  Carver cv(workspace, workspace_bytes);
  float* part = cv.take<float>((size_t)S * n);
  schnet_dw1_kernel<<<dim3((unsigned)S, (unsigned)ceil_div(K, 64)), 256, 0, st>>>(num_edges, per, d, ldd, centers, K, gamma,
                                                                                 dpre1, ld1, H, part);
  if (int rc = check_launch("schnet_dw1_kernel")) return rc;
  return colsum_final_launch(n, S, part, n, 1.f, accumulate ? 1.f : 0.f, dW1, st, "schnet_dw1 (partial sum)");
}

extern "C" int mvml_cfconv_agg(int64_t num_nodes, int64_t num_edges, const int32_t* rowptr, const int32_t* widx,
                               const int32_t* xidx, const float* X, int64_t ldx, const float* Wt, int64_t ldw, int H,
                               float* out, int64_t ldo, void* stream) {
  clear_error();
  if (int rc = check_schnet("cfconv_agg", H, 1)) return rc;
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31) && edges_ok(num_edges), "cfconv_agg: bad sizes %lld, %lld",
               (long long)num_nodes, (long long)num_edges);
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(rowptr != nullptr && row_ok(out, ldo, H),
               "cfconv_agg: rowptr is required; out must be 16-byte aligned with a pitch >= H that is a multiple of 4");
  MVML_REQUIRE(num_edges == 0 || (xidx != nullptr && row_ok(X, ldx, H) && row_ok(Wt, ldw, H)),
               "cfconv_agg: with edges, xidx is required and X and Wt must be 16-byte aligned with pitches >= H that are "
               "multiples of 4");
  const CfAggArgs a{num_nodes, rowptr, widx, xidx, X, ldx, Wt, ldw, H, out, ldo};
  const hipStream_t st = as_stream(stream);
  if (H <= 64)
    cfconv_agg_kernel<16, 4><<<(unsigned)ceil_div(num_nodes, 16), 256, 0, st>>>(a);
  else
    cfconv_agg_kernel<64, 4><<<(unsigned)ceil_div(num_nodes, 4), 256, 0, st>>>(a);
  return check_launch("cfconv_agg_kernel");
}

extern "C" int mvml_ssp_fwd(int64_t n, const float* x, float* y, void* stream) {
  clear_error();
  MVML_REQUIRE(n >= 0, "ssp_fwd: negative n");
  if (n == 0) return MVML_OK;
  MVML_REQUIRE(x != nullptr && y != nullptr, "ssp_fwd: x and y are required");
  ssp_fwd_kernel<<<(unsigned)std::min<int64_t>(ceil_div(n, 256), 8192), 256, 0, as_stream(stream)>>>(n, x, y);
  return check_launch("ssp_fwd_kernel");
}

extern "C" int mvml_ssp_bwd(int64_t n, const float* y, const float* g_y, float* g_x, void* stream) {
  clear_error();
  MVML_REQUIRE(n >= 0, "ssp_bwd: negative n");
  if (n == 0) return MVML_OK;
  MVML_REQUIRE(y != nullptr && g_y != nullptr && g_x != nullptr, "ssp_bwd: y, g_y and g_x are required");
  ssp_bwd_kernel<<<(unsigned)std::min<int64_t>(ceil_div(n, 256), 8192), 256, 0, as_stream(stream)>>>(n, y, g_y, g_x);
  return check_launch("ssp_bwd_kernel");
}
