// Weave's pair-update layer (dgllife 0.3.0 WeaveLayer; restated, parity with dgllife unpinned).  For an
// edge s = (u -> v) with state e_s, L = left_node_to_edge(x), R = right_node_to_edge(x):
//
//   third_s = relu(e_s W_ee^T + b_ee)
//   pair_s  = relu(L[u] + R[v]) + relu(R[u] + L[v])
//   e'_s    = relu([pair_s | third_s] W_ue^T + b_ue)
//   S[v]    = sum over v's in-slots of relu(e_s W_en^T + b_en)
//
// Every per-edge matrix is in in-CSR slot order.  All products are split-fp16 (gemm_common.h split2h8,
// three v_mfma_f32_16x16x32_f16 per step) on a tile of kWvTile = 128 consecutive slots: a workgroup of
// four waves, a wave owns 32 rows as two 16-row blocks and all output columns (up to eight 16-column
// blocks).  The A rows are loaded directly in fragment layout (row = lane & 15, k = 32 ks + 8 (lane >> 4)
// + j: two 16-B loads per k-step), every row split with its own power-of-two scale.  Any width in
// [1, 128]: K is zero-padded to 32s in the fragments and the weight images, N to 16-column blocks whose
// pad columns come out as exact zeros and are stored only up to the row's multiple of 4.
//
// weave_split_kernel: the weight images ([k-step][16-column block][{h, l}][64 lanes] x 16 B, as
// schnet.hip's), once per call: W_ee, W_en, W_ue's pair and third column blocks as they lie, and both
// transposed for the backward; the three maxima lead the file.  A panel (one k-step of up to four column
// blocks) is one contiguous run streamed through a two-slot LDS ring, one barrier per panel.
//
// weave_edge_fwd_kernel: product 1 gives third; it goes from accumulator layout to A-fragment layout
// through a wave-private LDS window.  pair is formed on load from the four gathered LR rows, in fragment
// layout.  Product 2 runs over the two k segments [pair | third] with one scale per row.  Only e' is
// written, and [pair | third] when a gradient is wanted.
// weave_edge_bwd_kernel: dpre = g * (e' > 0) formed on load and stored; dA = dpre W_ue on the transposed
// images, one column segment after the other; the first / second masks are recomputed from the LR rows
// with the forward's adds, third's mask is read from the saved operand.
// weave_e2n_fwd_kernel: relu(e W_en^T + b) of the tile goes to LDS, 64 columns at a time, and is summed
// per destination in slot order: a walker (64 columns, one of four) owns the runs that begin in its 32
// rows and follows each to its end.  A run inside the tile is stored; a run cut by the tile's first row
// leaves a head partial, one cut by its last row a tail partial, and weave_e2n_combine_kernel adds them
// in tile order (and writes the zero rows of atoms without in-edges).
// weave_e2n_bwd_kernel: the same pre-activation by the same device function (e_pre), so its mask has the
// forward's bits; dpre_en[s] = dS[dst s] * (pre > 0).
//
// No float atomics anywhere: bitwise repeatable.
#include "gemm_common.h"
#include "wave_ops.h"

namespace mvml {
namespace {

constexpr int kWvTile = 128;   // slots per workgroup: 4 waves x 2 MFMA row blocks of 16
constexpr int kWvPanel = 512;  // uint4 per ring slot: 4 column blocks x {h, l} x 64 lanes
constexpr int kWvMaxW = 128;
constexpr int kWvSumP = 68;    // LDS row pitch of the e2n tile (64 columns + 4)

__host__ __device__ inline int wv_ks(int K) { return (K + 31) / 32; }
__host__ __device__ inline int wv_nt(int N) { return (N + 15) / 16; }
__host__ __device__ inline int wv_r4(int n) { return (n + 3) / 4 * 4; }
inline size_t seg_vec(int N, int K) { return (size_t)wv_ks(K) * wv_nt(N) * 128; }

// [256 B: bits of max |W_ee|, |W_en|, |W_ue|][W_ee][W_en][W_ue pair][W_ue third][W_ue^T pair][W_ue^T third]
struct WvImage {
  const uint32_t* amax;
  const uint4* seg[6];
  // uint4 offsets of the six images behind the header, the total last
  static void offsets(int De, int Hee, int Hen, int Hne, int Heo, size_t (&off)[7]) {
    const int nk[6][2] = {{Hee, De}, {Hen, De}, {Heo, Hne}, {Heo, Hee}, {Hne, Heo}, {Hee, Heo}};
    off[0] = 0;
    for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + seg_vec(nk[i][0], nk[i][1]);
  }
  WvImage(const void* p, int De, int Hee, int Hen, int Hne, int Heo) : amax(static_cast<const uint32_t*>(p)) {
    size_t off[7];
    offsets(De, Hee, Hen, Hne, Heo, off);
    const uint4* q = reinterpret_cast<const uint4*>(static_cast<const char*>(p) + 256);
    for (int i = 0; i < 6; ++i) seg[i] = q + off[i];
  }
};

// B[k][n] = W[n sn + k sk] for n < N, k < K, else 0
struct WvSeg {
  const float* W;
  int64_t sn, sk;
  int N, K, am;
  int64_t off, cnt;  // uint4 offset of the image; threads (k-step, column block, lane)
};
struct WvSplitArgs {
  WvSeg s[6];
  const uint32_t* amax;
  uint4* img;
};

__global__ void __launch_bounds__(256) weave_split_kernel(WvSplitArgs a) {
  int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int i = 0;
  while (i < 6 && idx >= a.s[i].cnt) idx -= a.s[i++].cnt;
  if (i == 6) return;
  const WvSeg& g = a.s[i];
  const int NT = wv_nt(g.N), lane = (int)(idx & 63);
  const int64_t pn = idx >> 6;  // ks NT + nt
  const int nt = (int)(pn % NT), ks = (int)(pn / NT);
  const int n = nt * 16 + (lane & 15), k0 = ks * 32 + (lane >> 4) * 8;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (n < g.N && k0 + j < g.K) ? g.W[n * g.sn + (k0 + j) * g.sk] : 0.f;
  bf16x8 h, l;
  split2h8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), pow2f(amax_shift(a.amax[g.am])), h, l);
  uint4* dst = a.img + g.off + pn * 128 + lane;
  dst[0] = __builtin_bit_cast(uint4, h);
  dst[64] = __builtin_bit_cast(uint4, l);
}

// acc[rt][nt] += A(ks) B(ks, nt) over the nks k-steps of an image of NT column blocks, streamed panel by
// panel through the two-slot ring (schnet.hip sn_product with the A planes held in registers).  Every
// wave of the workgroup calls it; it ends on a barrier.
template <int NTB, int KSU>
__device__ __forceinline__ void wv_product(int nks, int NT, const uint4* __restrict__ img, uint4* ring, int tid, int lane,
                                           const f16x8 (&xh)[2][KSU], const f16x8 (&xl)[2][KSU], f32x4 (&acc)[2][NTB]) {
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
      if (tid + 256 * l < pcnt) ring[slot * kWvPanel + tid + 256 * l] = __builtin_bit_cast(uint4, pre[l]);
  };
  fetch(0, 0);
  park(0);
  __syncthreads();
  int buf = 0;
#pragma unroll
  for (int ks = 0; ks < KSU; ++ks) {
    if (ks < nks) {  // (uniform over the workgroup)
#pragma unroll
      for (int ng = 0; ng < NGB; ++ng) {
        if (4 * ng < NT) {
          const bool wrap = 4 * (ng + 1) >= NT, last = wrap && ks == nks - 1;
          if (!last) fetch(wrap ? ks + 1 : ks, wrap ? 0 : ng + 1);
          const uint4* pb = ring + buf * kWvPanel;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (4 * ng + j < NTB && 4 * ng + j < NT) {
              const f16x8 bh = __builtin_bit_cast(f16x8, pb[(2 * j) * 64 + lane]);
              const f16x8 bl = __builtin_bit_cast(f16x8, pb[(2 * j + 1) * 64 + lane]);
#pragma unroll
              for (int rt = 0; rt < 2; ++rt) {
                f32x4 c = acc[rt][(4 * ng + j) % NTB];
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl[rt][ks], bh, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[rt][ks], bl, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[rt][ks], bh, c, 0, 0, 0);
                acc[rt][(4 * ng + j) % NTB] = c;
              }
            }
          }
          if (!last) park(buf ^ 1);
          __syncthreads();
          buf ^= 1;
        }
      }
    }
  }
}

template <int NTB>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[2][NTB]) {
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nt = 0; nt < NTB; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ float relu(float x) { return x > 0.f ? x : 0.f; }

// The eight values k0 .. k0 + 7 of a row of n columns (16-byte aligned, pitch a multiple of 4 >= n);
// columns from n on are zero whatever the pitch holds.  k0 is a multiple of 8.
__device__ __forceinline__ void ld8(const float* row, int k0, int n, float (&v)[8]) {
  const float4 lo = k0 < n ? ld4(row + k0) : f4(0.f), hi = k0 + 4 < n ? ld4(row + k0 + 4) : f4(0.f);
  const float t[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = k0 + j < n ? t[j] : 0.f;
}
__device__ __forceinline__ float amax8(float m, const float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
  return m;
}
// eight values of a row, stored up to the row's multiple of 4 (n4)
__device__ __forceinline__ void st8(float* row, int k0, int n4, const float (&v)[8]) {
  if (k0 < n4) st4(row + k0, make_float4(v[0], v[1], v[2], v[3]));
  if (k0 + 4 < n4) st4(row + k0 + 4, make_float4(v[4], v[5], v[6], v[7]));
}
__device__ __forceinline__ void split8(const float (&v)[8], float sc, f16x8& h, f16x8& l) {
  bf16x8 hh, ll;
  split2h8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), sc, hh, ll);
  h = __builtin_bit_cast(f16x8, hh);
  l = __builtin_bit_cast(f16x8, ll);
}
// a row's four lane groups
__device__ __forceinline__ float groups_fmax(float m) {
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  return fmaxf(m, __shfl_xor(m, 32, 64));
}

// pre[rt][nt][r] = X[row] . W[col] + bias[col] of the wave's 32 rows (row e0 + 16 rt + 4 lg + r, column
// 16 nt + lr; columns from N on: exactly 0): the rows of X ([E][ldx], K columns) loaded in fragment layout,
// split per row, times the image; one fma per value.  The forward and the backward of mvml_weave_e2n_*
// both take their pre-activation from here.
template <int NTB, int KSU>
__device__ __forceinline__ void e_pre(const float* __restrict__ X, int64_t ldx, int K, int64_t E, int64_t e0,
                                      const uint4* __restrict__ img, int N, const float* __restrict__ bias, uint32_t wmax,
                                      uint4* ring, int tid, f32x4 (&acc)[2][NTB]) {
  const int lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  f16x8 xh[2][KSU], xl[2][KSU];
  int rsh[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t s = e0 + rt * 16 + lr;
    float v[KSU][8];
    float m = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) {
      const int k0 = ks * 32 + lg * 8;
      if (s < E && k0 < K) {
        ld8(X + s * ldx, k0, K, v[ks]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[ks][j] = 0.f;
      }
      m = amax8(m, v[ks]);
    }
    rsh[rt] = amax_shift(__float_as_uint(groups_fmax(m)));
    const float sc = pow2f(rsh[rt]);
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) split8(v[ks], sc, xh[rt][ks], xl[rt][ks]);
  }
  zero_acc(acc);
  wv_product<NTB, KSU>(wv_ks(K), wv_nt(N), img, ring, tid, lane, xh, xl, acc);
  const float uw = pow2f(-amax_shift(wmax));
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float usc = pow2f(-__shfl(rsh[rt], 4 * lg + r, 64)) * uw;  // (every lane takes part)
#pragma unroll
      for (int nt = 0; nt < NTB; ++nt) {
        const int col = 16 * nt + lr;
        acc[rt][nt][r] = __fmaf_rn(acc[rt][nt][r], usc, col < N ? bias[col] : 0.f);
      }
    }
}

struct WvEdgeFwdArgs {
  int64_t E;
  const int32_t *src, *dst;  // in_src, slot_dst
  const float* e;
  int64_t lde;
  const float* LR;  // [N][ldlr]: L in columns [0, Hne), R in [ro, ro + Hne)
  int64_t ldlr;
  int ro, De, Hee, Hne, Heo;
  const uint32_t* amax;
  const uint4 *img_ee, *img_p, *img_t;
  const float *b_ee, *b_ue;
  float* out;
  int64_t ldo;
  float* A;  // [E][lda] or null: pair in [0, Hne), third in [ao, ao + Hee)
  int64_t lda;
  int ao;
};

// NTB: the 16-column blocks the instance holds accumulators for; every width <= 16 NTB.
template <int NTB>
__global__ void __launch_bounds__(256) weave_edge_fwd_kernel(WvEdgeFwdArgs a) {
  constexpr int KSU = NTB / 2, P = NTB * 16 + 4;  // window row pitch; column 16 NTB of a row: its third maximum
  __shared__ uint4 ring[2 * kWvPanel];
  __shared__ float win[4][16 * P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * kWvTile + wave * 32;
  f32x4 acc[2][NTB];
  e_pre<NTB, KSU>(a.e, a.lde, a.De, a.E, e0, a.img_ee, a.Hee, a.b_ee, a.amax[0], ring, tid, acc);

  f16x8 ph[2][KSU], pl[2][KSU], th[2][KSU], tl[2][KSU];
  int rsh[2];
  float* w = win[wave];
  const int Hne = a.Hne, Hee = a.Hee, ao = a.ao;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < NTB; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = relu(acc[rt][nt][r]);
        m[r] = fmaxf(m[r], v);
        w[(4 * lg + r) * P + 16 * nt + lr] = v;
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o, 64));
      if (lr == 0) w[(4 * lg + r) * P + 16 * NTB] = m[r];
    }
    wave_sync_lds();
    const int64_t s = e0 + rt * 16 + lr;
    const bool live = s < a.E;
    const float* ur = a.LR + (int64_t)(live ? a.src[s] : 0) * a.ldlr;
    const float* vr = a.LR + (int64_t)(live ? a.dst[s] : 0) * a.ldlr;
    float pv[KSU][8], tv[KSU][8];
    float mp = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) {
      const int k0 = ks * 32 + lg * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) pv[ks][j] = 0.f;
      if (live && k0 < Hne) {
        float lu[8], rv[8], ru[8], lv[8];
        ld8(ur, k0, Hne, lu);
        ld8(vr + a.ro, k0, Hne, rv);
        ld8(ur + a.ro, k0, Hne, ru);
        ld8(vr, k0, Hne, lv);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          pv[ks][j] = __fadd_rn(relu(__fadd_rn(lu[j], rv[j])), relu(__fadd_rn(ru[j], lv[j])));
      }
      mp = amax8(mp, pv[ks]);
      const float4 lo = ld4(w + lr * P + k0), hi = ld4(w + lr * P + k0 + 4);  // (columns from Hee on are 0)
      const float t[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) tv[ks][j] = t[j];
      if (a.A != nullptr && live) {
        st8(a.A + s * a.lda, k0, ao, pv[ks]);
        st8(a.A + s * a.lda + ao, k0, wv_r4(Hee), tv[ks]);
      }
    }
    const float mrow = fmaxf(groups_fmax(mp), w[lr * P + 16 * NTB]);
    rsh[rt] = amax_shift(__float_as_uint(mrow));
    const float sc = pow2f(rsh[rt]);
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) {
      split8(pv[ks], sc, ph[rt][ks], pl[rt][ks]);
      split8(tv[ks], sc, th[rt][ks], tl[rt][ks]);
    }
    wave_sync_lds();  // the reads are done before the next row block's writes
  }
  zero_acc(acc);
  const int NT = wv_nt(a.Heo);
  wv_product<NTB, KSU>(wv_ks(Hne), NT, a.img_p, ring, tid, lane, ph, pl, acc);
  wv_product<NTB, KSU>(wv_ks(Hee), NT, a.img_t, ring, tid, lane, th, tl, acc);
  const float uw = pow2f(-amax_shift(a.amax[2]));
  const int Ho4 = wv_r4(a.Heo);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float usc = pow2f(-__shfl(rsh[rt], 4 * lg + r, 64)) * uw;  // (every lane takes part)
      const int64_t s = e0 + rt * 16 + 4 * lg + r;
      if (s >= a.E) continue;
#pragma unroll
      for (int nt = 0; nt < NTB; ++nt) {
        const int col = 16 * nt + lr;
        if (col < Ho4) a.out[s * a.ldo + col] = relu(__fmaf_rn(acc[rt][nt][r], usc, col < a.Heo ? a.b_ue[col] : 0.f));
      }
    }
}

struct WvEdgeBwdArgs {
  int64_t E;
  const int32_t *src, *dst;
  const float* g;  // dL/de' [E][ldg]
  int64_t ldg;
  const float* out;  // e' [E][ldo]
  int64_t ldo;
  const float* A;
  int64_t lda;
  int ao;
  const float* LR;
  int64_t ldlr;
  int ro, Hee, Hne, Heo;
  const uint32_t* amax;
  const uint4 *img_pt, *img_tt;
  float* dpre;  // [E][ldp], Heo columns
  int64_t ldp;
  float* dfs;  // [E][ldf]: dfirst in [0, Hne), dsecond in [fo, fo + Hne)
  int64_t ldf;
  int fo;
  float* dthird;  // [E][ldt], Hee columns
  int64_t ldt;
};

template <int NTB>
__global__ void __launch_bounds__(256) weave_edge_bwd_kernel(WvEdgeBwdArgs a) {
  constexpr int KSU = NTB / 2;
  __shared__ uint4 ring[2 * kWvPanel];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * kWvTile + wave * 32;
  const int Heo = a.Heo, Hne = a.Hne, Hee = a.Hee;
  f16x8 xh[2][KSU], xl[2][KSU];
  int rsh[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t s = e0 + rt * 16 + lr;
    const bool live = s < a.E;
    float d[KSU][8];
    float m = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) {
      const int k0 = ks * 32 + lg * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) d[ks][j] = 0.f;
      if (live && k0 < Heo) {  // dpre = g * (e' > 0): g's bits or +0, formed and stored in fragment layout
        float gv[8], ov[8];
        ld8(a.g + s * a.ldg, k0, Heo, gv);
        ld8(a.out + s * a.ldo, k0, Heo, ov);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[ks][j] = ov[j] > 0.f ? gv[j] : 0.f;
        st8(a.dpre + s * a.ldp, k0, wv_r4(Heo), d[ks]);
      }
      m = amax8(m, d[ks]);
    }
    rsh[rt] = amax_shift(__float_as_uint(groups_fmax(m)));
    const float sc = pow2f(rsh[rt]);
#pragma unroll
    for (int ks = 0; ks < KSU; ++ks) split8(d[ks], sc, xh[rt][ks], xl[rt][ks]);
  }
  const float uw = pow2f(-amax_shift(a.amax[2]));
  f32x4 acc[2][NTB];
  zero_acc(acc);
  wv_product<NTB, KSU>(wv_ks(Heo), wv_nt(Hne), a.img_pt, ring, tid, lane, xh, xl, acc);
  const int Hn4 = wv_r4(Hne);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float usc = pow2f(-__shfl(rsh[rt], 4 * lg + r, 64)) * uw;  // (every lane takes part)
      const int64_t s = e0 + rt * 16 + 4 * lg + r;
      if (s >= a.E) continue;
      const float* ur = a.LR + (int64_t)a.src[s] * a.ldlr;
      const float* vr = a.LR + (int64_t)a.dst[s] * a.ldlr;
#pragma unroll
      for (int nt = 0; nt < NTB; ++nt) {
        const int col = 16 * nt + lr;
        if (col < Hn4) {  // (pad columns: LR holds zeros there, and the product is 0)
          const float da = acc[rt][nt][r] * usc;
          a.dfs[s * a.ldf + col] = __fadd_rn(ur[col], vr[a.ro + col]) > 0.f ? da : 0.f;
          a.dfs[s * a.ldf + a.fo + col] = __fadd_rn(ur[a.ro + col], vr[col]) > 0.f ? da : 0.f;
        }
      }
    }
  zero_acc(acc);
  wv_product<NTB, KSU>(wv_ks(Heo), wv_nt(Hee), a.img_tt, ring, tid, lane, xh, xl, acc);
  const int He4 = wv_r4(Hee);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float usc = pow2f(-__shfl(rsh[rt], 4 * lg + r, 64)) * uw;
      const int64_t s = e0 + rt * 16 + 4 * lg + r;
      if (s >= a.E) continue;
#pragma unroll
      for (int nt = 0; nt < NTB; ++nt) {
        const int col = 16 * nt + lr;
        if (col < He4) a.dthird[s * a.ldt + col] = a.A[s * a.lda + a.ao + col] > 0.f ? acc[rt][nt][r] * usc : 0.f;
      }
    }
}

struct WvE2nArgs {
  int64_t E;
  const int32_t *rowptr, *dst;  // in_rowptr, slot_dst
  const float* e;
  int64_t lde;
  int De, Hen;
  const uint32_t* amax;
  const uint4* img;
  const float* b;
  float* S;  // forward: [N][lds]; backward: dS
  int64_t lds;
  float *head, *tail;  // forward: [tiles][Hen] partials
  float* dpre;         // backward: [E][ldd]
  int64_t ldd;
};

template <int NTB>
__global__ void __launch_bounds__(256) weave_e2n_fwd_kernel(WvE2nArgs a) {
  constexpr int KSU = NTB / 2, NGB = (NTB + 3) / 4;
  __shared__ uint4 ring[2 * kWvPanel];
  __shared__ float tile[kWvTile * kWvSumP];
  __shared__ int dsts[kWvTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * kWvTile, e0 = t0 + wave * 32;
  const int n = (int)min((int64_t)kWvTile, a.E - t0), Hen = a.Hen, NT = wv_nt(Hen);
  if (tid < kWvTile) dsts[tid] = tid < n ? a.dst[t0 + tid] : -1;
  f32x4 acc[2][NTB];
  e_pre<NTB, KSU>(a.e, a.lde, a.De, a.E, e0, a.img, Hen, a.b, a.amax[1], ring, tid, acc);
  const int c = tid & 63, q = tid >> 6;
#pragma unroll
  for (int ng = 0; ng < NGB; ++ng) {
    if (4 * ng < NT) {  // (uniform over the workgroup)
      __syncthreads();  // the previous pass's reads are done
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * ng + j < NTB) {
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              tile[(wave * 32 + rt * 16 + 4 * lg + r) * kWvSumP + 16 * j + lr] = relu(acc[rt][(4 * ng + j) % NTB][r]);
        }
      __syncthreads();
      const int col = 64 * ng + c;
      if (col < Hen) {
        const int end = min(32 * q + 32, n);
        int r = 32 * q;
        while (r > 0 && r < end && dsts[r] == dsts[r - 1]) ++r;  // a run that began in an earlier walker's rows
        while (r < end) {
          const int v = dsts[r];
          float sum = tile[r * kWvSumP + c];
          int r2 = r + 1;
          for (; r2 < n && dsts[r2] == v; ++r2) sum = __fadd_rn(sum, tile[r2 * kWvSumP + c]);  // slot order
          if (a.rowptr[v] < t0)
            a.head[(int64_t)blockIdx.x * Hen + col] = sum;
          else if (a.rowptr[v + 1] > t0 + kWvTile)
            a.tail[(int64_t)blockIdx.x * Hen + col] = sum;
          else
            a.S[(int64_t)v * a.lds + col] = sum;
          r = r2;
        }
      }
    }
  }
}

// One thread per (atom, column): an atom without in-edges gets +0, a run that spans tiles t0 .. t1 its tail
// partial of t0 plus the head partials of t0 + 1 .. t1 in that order; any other row is already stored.
__global__ void __launch_bounds__(256)
weave_e2n_combine_kernel(int64_t N, const int32_t* __restrict__ rowptr, const float* __restrict__ head,
                         const float* __restrict__ tail, int Hen, float* __restrict__ S, int64_t lds) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t v = idx / Hen;
  const int col = (int)(idx - v * Hen);
  if (v >= N) return;
  const int b = rowptr[v], e = rowptr[v + 1];
  if (b == e) {
    S[v * lds + col] = 0.f;
    return;
  }
  const int t0 = b / kWvTile, t1 = (e - 1) / kWvTile;
  if (t0 == t1) return;
  float sum = tail[(int64_t)t0 * Hen + col];
  for (int t = t0 + 1; t <= t1; ++t) sum = __fadd_rn(sum, head[(int64_t)t * Hen + col]);
  S[v * lds + col] = sum;
}

template <int NTB>
__global__ void __launch_bounds__(256) weave_e2n_bwd_kernel(WvE2nArgs a) {
  constexpr int KSU = NTB / 2;
  __shared__ uint4 ring[2 * kWvPanel];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * kWvTile + wave * 32;
  f32x4 acc[2][NTB];
  e_pre<NTB, KSU>(a.e, a.lde, a.De, a.E, e0, a.img, a.Hen, a.b, a.amax[1], ring, tid, acc);
  const int H4 = wv_r4(a.Hen);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t s = e0 + rt * 16 + 4 * lg + r;
      if (s >= a.E) continue;
      const float* gr = a.S + (int64_t)a.dst[s] * a.lds;
#pragma unroll
      for (int nt = 0; nt < NTB; ++nt) {
        const int col = 16 * nt + lr;
        if (col < H4) a.dpre[s * a.ldd + col] = (col < a.Hen && acc[rt][nt][r] > 0.f) ? gr[col] : 0.f;
      }
    }
}

// dst[eid[s]] = src[s] (scatter) or dst[s] = src[eid[s]]: slot order <-> edge-id order, a permutation
__global__ void __launch_bounds__(256)
weave_permute_kernel(int64_t E, int cols, const int32_t* __restrict__ eid, const float* __restrict__ src, int64_t lds,
                     float* __restrict__ dst, int64_t ldd, int scatter) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t s = idx / cols;
  const int c = (int)(idx - s * cols);
  if (s >= E) return;
  const int64_t o = eid[s];
  if (scatter)
    dst[o * ldd + c] = src[s * lds + c];
  else
    dst[s * ldd + c] = src[o * lds + c];
}

bool width_ok(int w) { return w >= 1 && w <= kWvMaxW; }
bool edges_ok(int64_t E) { return E >= 0 && E < (int64_t(1) << 31) - kWvTile; }
bool nodes_ok(int64_t N) { return N >= 0 && N < (int64_t(1) << 31); }
int check_widths(const char* who, int De, int Hee, int Hen, int Hne, int Heo) {
  MVML_REQUIRE(width_ok(De) && width_ok(Hee) && width_ok(Hen) && width_ok(Hne) && width_ok(Heo),
               "%s: every width must be in [1, %d] (got edge_in %d, edge_edge %d, edge_node %d, node_edge %d, edge_out %d)",
               who, kWvMaxW, De, Hee, Hen, Hne, Heo);
  return MVML_OK;
}

template <typename Fn>
int by_width(int w, Fn&& fn) {  // the instance whose blocks cover the widest operand
  return w <= 32 ? fn(std::integral_constant<int, 2>{}) : w <= 64 ? fn(std::integral_constant<int, 4>{})
                                                                   : fn(std::integral_constant<int, 8>{});
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" size_t mvml_weave_image_bytes(int De, int Hee, int Hen, int Hne, int Heo) {
  if (!(width_ok(De) && width_ok(Hee) && width_ok(Hen) && width_ok(Hne) && width_ok(Heo))) return 0;
  size_t off[7];
  WvImage::offsets(De, Hee, Hen, Hne, Heo, off);
  return 256 + 16 * off[6];
}

extern "C" int mvml_weave_split_w(int De, int Hee, int Hen, int Hne, int Heo, const float* W_ee, const float* W_en,
                                  const float* W_ue, void* image, void* stream) {
  clear_error();
  if (int rc = check_widths("weave_split_w", De, Hee, Hen, Hne, Heo)) return rc;
  MVML_REQUIRE(W_en != nullptr && (W_ee == nullptr) == (W_ue == nullptr) && image != nullptr && aligned16(image),
               "weave_split_w: W_en and a 16-byte aligned image are required; W_ee and W_ue go together");
  const hipStream_t st = as_stream(stream);
  uint32_t* amax = static_cast<uint32_t*>(image);
  const int K2 = Hne + Hee;
  if (int rc = absmax_launch(Hen, De, W_en, De, amax + 1, false, st)) return rc;
  if (W_ee != nullptr) {
    if (int rc = absmax_launch(Hee, De, W_ee, De, amax, false, st)) return rc;
    if (int rc = absmax_launch(Heo, K2, W_ue, K2, amax + 2, false, st)) return rc;
  }
  WvImage im(image, De, Hee, Hen, Hne, Heo);
  const uint4* base = im.seg[0];
  const float* Wt = W_ue ? W_ue + Hne : nullptr;
  WvSplitArgs a{{{W_ee, De, 1, Hee, De, 0, 0, 0}, {W_en, De, 1, Hen, De, 1, 0, 0}, {W_ue, K2, 1, Heo, Hne, 2, 0, 0},
                 {Wt, K2, 1, Heo, Hee, 2, 0, 0}, {W_ue, 1, K2, Hne, Heo, 2, 0, 0}, {Wt, 1, K2, Hee, Heo, 2, 0, 0}},
                im.amax, const_cast<uint4*>(base)};
  int64_t total = 0;
  for (int i = 0; i < 6; ++i) {
    a.s[i].off = im.seg[i] - base;
    a.s[i].cnt = a.s[i].W ? (int64_t)seg_vec(a.s[i].N, a.s[i].K) / 2 : 0;
    total += a.s[i].cnt;
  }
  weave_split_kernel<<<(unsigned)ceil_div(total, 256), 256, 0, st>>>(a);
  return check_launch("weave_split_kernel");
}

extern "C" int mvml_weave_edge_fwd(int64_t num_nodes, int64_t num_edges, const int32_t* in_src, const int32_t* slot_dst,
                                   const float* e, int64_t lde, int De, const float* LR, int64_t ldlr, int r_off, int Hne,
                                   int Hee, int Hen, int Heo, const void* image, const float* b_ee, const float* b_ue,
                                   float* out, int64_t ldo, float* A, int64_t lda, void* stream) {
  clear_error();
  if (int rc = check_widths("weave_edge_fwd", De, Hee, Hen, Hne, Heo)) return rc;
  MVML_REQUIRE(nodes_ok(num_nodes) && edges_ok(num_edges), "weave_edge_fwd: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(in_src != nullptr && slot_dst != nullptr && image != nullptr && aligned16(image) && b_ee != nullptr &&
                   b_ue != nullptr,
               "weave_edge_fwd: in_src, slot_dst, a 16-byte aligned image, b_ee and b_ue are required");
  const int Hq = wv_r4(Hne), ao = Hq;
  MVML_REQUIRE(row_ok(e, lde, De) && row_ok(out, ldo, Heo) && r_off >= Hq && r_off % 4 == 0 && row_ok(LR, ldlr, r_off + Hq) &&
                   (A == nullptr || row_ok(A, lda, ao + wv_r4(Hee))),
               "weave_edge_fwd: e, LR, out and A must be 16-byte aligned with pitches that are multiples of 4 and hold "
               "their columns (LR: r_off a multiple of 4 >= node_edge, pitch >= r_off + node_edge; A: both parts, each "
               "rounded up to 4)");
  WvImage im(image, De, Hee, Hen, Hne, Heo);
  const WvEdgeFwdArgs a{num_edges, in_src, slot_dst, e,    lde,  LR,  ldlr, r_off, De,  Hee, Hne, Heo,
                        im.amax,   im.seg[0], im.seg[2], im.seg[3], b_ee, b_ue, out, ldo, A, lda, ao};
  const unsigned grid = (unsigned)ceil_div(num_edges, kWvTile);
  const hipStream_t st = as_stream(stream);
  by_width(std::max(std::max(De, Hee), std::max(Hne, Heo)), [&](auto n) {
    weave_edge_fwd_kernel<decltype(n)::value><<<grid, 256, 0, st>>>(a);
    return MVML_OK;
  });
  return check_launch("weave_edge_fwd_kernel");
}

extern "C" int mvml_weave_edge_bwd(int64_t num_nodes, int64_t num_edges, const int32_t* in_src, const int32_t* slot_dst,
                                   const float* g_out, int64_t ldg, const float* out, int64_t ldo, const float* A,
                                   int64_t lda, const float* LR, int64_t ldlr, int r_off, int De, int Hne, int Hee,
                                   int Hen, int Heo, const void* image, float* dpre, int64_t ldp, float* dfs, int64_t ldf,
                                   float* dthird, int64_t ldt, void* stream) {
  clear_error();
  if (int rc = check_widths("weave_edge_bwd", De, Hee, Hen, Hne, Heo)) return rc;
  MVML_REQUIRE(nodes_ok(num_nodes) && edges_ok(num_edges), "weave_edge_bwd: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(in_src != nullptr && slot_dst != nullptr && image != nullptr && aligned16(image),
               "weave_edge_bwd: in_src, slot_dst and a 16-byte aligned image are required");
  const int Hq = wv_r4(Hne), ao = Hq;
  MVML_REQUIRE(row_ok(g_out, ldg, Heo) && row_ok(out, ldo, Heo) && row_ok(A, lda, ao + wv_r4(Hee)) && r_off >= Hq &&
                   r_off % 4 == 0 && row_ok(LR, ldlr, r_off + Hq) && row_ok(dpre, ldp, Heo) && row_ok(dfs, ldf, 2 * Hq) &&
                   row_ok(dthird, ldt, Hee),
               "weave_edge_bwd: g_out, out, A, LR, dpre, dfs and dthird must be 16-byte aligned with pitches that are "
               "multiples of 4 and hold their columns (dfs: twice node_edge rounded up to 4)");
  WvImage im(image, De, Hee, Hen, Hne, Heo);
  const WvEdgeBwdArgs a{num_edges, in_src, slot_dst, g_out, ldg, out,     ldo,       A,         lda,  ao,  LR,  ldlr, r_off,
                        Hee,       Hne,    Heo,      im.amax,   im.seg[4], im.seg[5], dpre, ldp, dfs, ldf,  Hq,  dthird, ldt};
  const unsigned grid = (unsigned)ceil_div(num_edges, kWvTile);
  const hipStream_t st = as_stream(stream);
  by_width(std::max(Heo, std::max(Hne, Hee)), [&](auto n) {
    weave_edge_bwd_kernel<decltype(n)::value><<<grid, 256, 0, st>>>(a);
    return MVML_OK;
  });
  return check_launch("weave_edge_bwd_kernel");
}

extern "C" size_t mvml_weave_e2n_workspace_size(int64_t num_edges, int Hen) {
  if (num_edges < 0 || !width_ok(Hen)) return 0;
  return 2 * carve_size((size_t)ceil_div(std::max<int64_t>(num_edges, 1), kWvTile) * Hen * 4) + 256;
}

extern "C" int mvml_weave_e2n_fwd(int64_t num_nodes, int64_t num_edges, const int32_t* in_rowptr, const int32_t* slot_dst,
                                  const float* e, int64_t lde, int De, int Hee, int Hen, int Hne, int Heo,
                                  const void* image, const float* b_en, float* S, int64_t lds, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  clear_error();
  if (int rc = check_widths("weave_e2n_fwd", De, Hee, Hen, Hne, Heo)) return rc;
  MVML_REQUIRE(nodes_ok(num_nodes) && edges_ok(num_edges), "weave_e2n_fwd: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(in_rowptr != nullptr && S != nullptr && lds >= Hen && lds < (int64_t(1) << 28),
               "weave_e2n_fwd: in_rowptr and S with a pitch >= edge_node are required");
  MVML_REQUIRE(num_edges == 0 || (slot_dst != nullptr && image != nullptr && aligned16(image) && b_en != nullptr &&
                                  row_ok(e, lde, De)),
               "weave_e2n_fwd: with edges, slot_dst, a 16-byte aligned image and b_en are required, and e must be 16-byte "
               "aligned with a pitch >= edge_in that is a multiple of 4");
  const size_t need = mvml_weave_e2n_workspace_size(num_edges, Hen);
  if (num_edges > 0 && (workspace == nullptr || workspace_bytes < need)) {
    set_error("weave_e2n_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  float *head = nullptr, *tail = nullptr;
  if (num_edges > 0) {
    const size_t tiles = (size_t)ceil_div(num_edges, kWvTile);
    Carver cv(workspace, workspace_bytes);
    head = cv.take<float>(tiles * Hen);
    tail = cv.take<float>(tiles * Hen);
    WvImage im(image, De, Hee, Hen, Hne, Heo);
    const WvE2nArgs a{num_edges, in_rowptr, slot_dst, e, lde, De, Hen, im.amax, im.seg[1], b_en, S, lds, head, tail, nullptr, 0};
    by_width(std::max(De, Hen), [&](auto n) {
      weave_e2n_fwd_kernel<decltype(n)::value><<<(unsigned)tiles, 256, 0, st>>>(a);
      return MVML_OK;
    });
    if (int rc = check_launch("weave_e2n_fwd_kernel")) return rc;
  }
  weave_e2n_combine_kernel<<<(unsigned)ceil_div(num_nodes * Hen, 256), 256, 0, st>>>(num_nodes, in_rowptr, head, tail, Hen, S,
                                                                                   lds);
  return check_launch("weave_e2n_combine_kernel");
}

extern "C" int mvml_weave_e2n_bwd(int64_t num_nodes, int64_t num_edges, const int32_t* slot_dst, const float* e,
                                  int64_t lde, int De, int Hee, int Hen, int Hne, int Heo, const void* image,
                                  const float* b_en, const float* dS, int64_t ldds, float* dpre, int64_t ldd,
                                  void* stream) {
  clear_error();
  if (int rc = check_widths("weave_e2n_bwd", De, Hee, Hen, Hne, Heo)) return rc;
  MVML_REQUIRE(nodes_ok(num_nodes) && edges_ok(num_edges), "weave_e2n_bwd: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(slot_dst != nullptr && image != nullptr && aligned16(image) && b_en != nullptr && dS != nullptr &&
                   ldds >= Hen && ldds < (int64_t(1) << 28),
               "weave_e2n_bwd: slot_dst, a 16-byte aligned image, b_en and dS with a pitch >= edge_node are required");
  MVML_REQUIRE(row_ok(e, lde, De) && row_ok(dpre, ldd, Hen),
               "weave_e2n_bwd: e and dpre must be 16-byte aligned with pitches that are multiples of 4 and hold their columns");
  WvImage im(image, De, Hee, Hen, Hne, Heo);
  const WvE2nArgs a{num_edges, nullptr, slot_dst, e, lde, De, Hen, im.amax, im.seg[1], b_en, const_cast<float*>(dS), ldds,
                    nullptr,   nullptr, dpre,     ldd};
  const hipStream_t st = as_stream(stream);
  by_width(std::max(De, Hen), [&](auto n) {
    weave_e2n_bwd_kernel<decltype(n)::value><<<(unsigned)ceil_div(num_edges, kWvTile), 256, 0, st>>>(a);
    return MVML_OK;
  });
  return check_launch("weave_e2n_bwd_kernel");
}

extern "C" int mvml_weave_permute_rows(int64_t num_edges, int cols, const int32_t* in_eid, const float* src, int64_t lds,
                                       float* dst, int64_t ldd, int scatter, void* stream) {
  clear_error();
  MVML_REQUIRE(edges_ok(num_edges) && cols >= 1 && cols <= (1 << 20), "weave_permute_rows: bad sizes %lld, %d",
               (long long)num_edges, cols);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(in_eid != nullptr && src != nullptr && dst != nullptr && src != dst && lds >= cols && ldd >= cols,
               "weave_permute_rows: in_eid and distinct src and dst with pitches >= cols are required");
  weave_permute_kernel<<<(unsigned)ceil_div(num_edges * cols, 256), 256, 0, as_stream(stream)>>>(num_edges, cols, in_eid, src,
                                                                                                 lds, dst, ldd, scatter);
  return check_launch("weave_permute_kernel");
}
