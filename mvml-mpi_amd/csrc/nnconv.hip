// MPNN's edge-network convolution (dgl 0.9.1 NNConv with a sum aggregator, dgllife 0.3.0 MPNNGNN;
// restated, parity with dgllife unpinned) without the per-edge weight matrices in memory.
//
//   W_e = view(z_e W2^T + b2, [D, D]),  m_e = h_u W_e,  out_v = sum_{e: u -> v} m_e + bias
//
// Re-associated over the rows i of W_e (W2_i = the [H, D] slice of W2 that makes row i):
//
//   m_e = sum_i h_u[i] (z_e W2_i)  (+ h_u view(b2): node-level, on the GEMM)
//
// so a tile of T edges runs D small products C_i = Z_tile [T, H] x W2_i [H, D] on the matrix pipe
// and folds each into its accumulators with one fma per element, acc += h[:, i] * C_i.  The data
// gradients have the same shape with the roles of H and D swapped (C'_i = dM_tile [T, D] x W2_i^T
// [D, H]; dz += h[:, i] * C'_i, dh[:, i] = <z, C'_i>), so ONE kernel template serves both.
//
// nnconv_tile_kernel: a workgroup of four waves owns kNnTile = 128 consecutive in-CSR slots and (grid
// y) 64 of the product's columns; a wave owns 32 of the rows as two 16-row MFMA blocks.  Its A rows
// (z, or the gathered dOut rows) are read ONCE, scaled per row, split into two fp16 planes
// (gemm_common.h split2h8) and stay in registers as MFMA fragments for all D values of i.  W2 is
// split once per call into an image in fragment order (nnconv_split_kernel): panel (i, 16-column
// block) = KS k-steps x {h, l} x 64 lanes x 16 B, so a panel is one contiguous run that the four
// waves stream from L2 through a two-slot LDS ring, one barrier per panel.  Per panel and row block:
// 3 KS v_mfma_f32_16x16x32_f16 (l h, h l, h h), then the fold on the four accumulator registers.
// The source rows h[src] are staged 16 values of i at a time.  K is padded to KS * 32, KS in
// {1, 2, 4, 8} (zeros in the image and the fragments).  The scales (2^-shift of the row, 2^-shift
// of W2) commute with the sum over i and are applied once, as the rows leave.
//
// The forward writes per-edge rows [E][D] and nnconv_rows_sum_kernel adds a destination's slots in
// slot order (+ bias); the backward writes dz in place (accumulate: read-add-write, one owner per
// element) and per-edge dh partials, one [E][D] slab per 64-column group, which the same sum kernel
// adds over a source atom's out-edges.  No float atomics anywhere: bitwise repeatable, and a row's
// bits do not depend on the batch around it.
//
// nnconv_wgrad_kernel: dW2[(i, o), k] = sum_e (h[src e][i] dM[e][o]) z[e][k] contracts over the
// edges, so both operands are edge-major in memory: fp32 MFMA (v_mfma_f32_16x16x4f32) takes them
// in that layout (A and B lanes both run along the 16 contiguous o / k), where the split-fp16 form
// needs two LDS transposes and a re-split of h_i * dM per i.  Grid (i, edge range): a workgroup
// stages 32 edges of dM, z and h[:, i] in LDS, wave w owns the 16-column blocks w, w + 4, ... of H
// and all D / 16 row blocks.  The edge ranges' partials are summed in fixed order
// (colsum_final_launch), onto dW2 when accumulating.
#include "gemm_common.h"

namespace mvml {
namespace {

constexpr int kNnTile = 128;  // edges per workgroup: 4 waves x 2 MFMA row blocks of 16
constexpr int kNnCols = 64;   // product columns per workgroup: 4 MFMA column blocks of 16
constexpr int kNnIc = 16;     // values of i per staged h chunk
constexpr int kNnHs = kNnIc + 4;  // LDS row pitch of the chunk (the four row groups hit distinct banks)
constexpr int kNnWgE = 32;    // edges per staged chunk of the weight gradient

__device__ __forceinline__ float4 nn_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void nn_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__host__ __device__ inline int nn_ks(int K) { return K <= 32 ? 1 : K <= 64 ? 2 : K <= 128 ? 4 : 8; }
// LDS row pitch of `x` floats (x % 16 == 0) with pitch % 64 == 16: rows e, e + 1, e + 2, e + 3 of a
// 16-float column block fall into distinct banks
__host__ __device__ inline int nn_pitch(int x) { return x + (80 - x % 64) % 64; }

// The images of W2 [D * D][H]: one thread per (panel, k-step, lane), eight k values each.
//   forward  (N = D, K = H): B_i[k][n] = W2[(i D + n) H + k]
//   backward (N = H, K = D): B_i[k][n] = W2[(i D + k) H + n]
__global__ void __launch_bounds__(256)
nnconv_split_kernel(int D, int H, const float* __restrict__ W2, const uint32_t* __restrict__ amax,
                    uint4* __restrict__ img_f, uint4* __restrict__ img_b) {
  const int ksf = nn_ks(H), ksb = nn_ks(D);
  const int64_t nf = (int64_t)D * (D / 16) * ksf * 64, nb = (int64_t)D * (H / 16) * ksb * 64;
  int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nf + nb) return;
  const bool bwd = idx >= nf;
  if (bwd) idx -= nf;
  const int KS = bwd ? ksb : ksf, NT = (bwd ? H : D) / 16, K = bwd ? D : H;
  const int lane = (int)(idx & 63);
  const int ks = (int)((idx >> 6) % KS);
  const int64_t pn = (idx >> 6) / KS;  // panel i NT + nt
  const int nt = (int)(pn % NT), i = (int)(pn / NT);
  const int n = nt * 16 + (lane & 15), k0 = ks * 32 + (lane >> 4) * 8;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    v[j] = k < K ? (bwd ? W2[((int64_t)i * D + k) * H + n] : W2[((int64_t)i * D + n) * H + k]) : 0.f;
  }
  bf16x8 h, l;
  split2h8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), pow2f(amax_shift(*amax)), h, l);
  uint4* dst = (bwd ? img_b : img_f) + (pn * KS + ks) * 128 + lane;
  dst[0] = __builtin_bit_cast(uint4, h);
  dst[64] = __builtin_bit_cast(uint4, l);
}

// slot_dst[s] = v for the slots s of v's in-CSR row.
__global__ void __launch_bounds__(256)
nnconv_slot_dst_kernel(int64_t N, const int32_t* __restrict__ rowptr, int32_t* __restrict__ slot_dst) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  for (int s = rowptr[v]; s < rowptr[v + 1]; ++s) slot_dst[s] = (int32_t)v;
}

struct NnTileArgs {
  int64_t E;
  const float* A;          // MFMA A rows: z [E][lda] (forward), dOut [N][lda] (backward)
  int64_t lda;
  const int32_t* row_id;   // backward: slot -> destination atom (the A row); forward: NULL (the slot)
  int K;                   // A's columns: H (forward), D (backward)
  const int32_t* src;      // in_src
  const float* h;          // [N][ldh]
  int64_t ldh;
  int D;
  const uint4* img;        // this direction's image
  int NT;                  // its 16-column blocks: D / 16 (forward), H / 16 (backward)
  const uint32_t* amax_w;  // bits of max |W2|
  float* out;              // forward: per-edge rows [E][ldo]; backward: dz [E][ldo]
  int64_t ldo;
  int accumulate;          // backward: dz += instead of =
  const float* z;          // backward: z [E][ldz] once more, in the accumulators' layout
  int64_t ldz;
  float* dh;               // backward: [column groups][E][D]
};

template <int KS, bool BWD>
__global__ void __launch_bounds__(256) nnconv_tile_kernel(NnTileArgs a) {
  constexpr int PV = KS * 128;             // uint4 per panel
  constexpr int NL = (PV + 255) / 256;     // uint4 per thread and panel
  __shared__ uint4 ring[2 * PV];
  __shared__ float hs[kNnTile * kNnHs];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * kNnTile;
  const int nt0 = blockIdx.y * 4, ntc = min(4, a.NT - nt0);
  const int D = a.D;

  // the wave's A fragments: row block rt, row 16 rt + lr, k = 32 ks + 8 lg + (0..7)
  f16x8 ah[2][KS], al[2][KS];
  int rsh[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t s = e0 + wave * 32 + rt * 16 + lr;
    const float* ar = nullptr;
    if (s < a.E) ar = a.A + (int64_t)(BWD ? a.row_id[s] : s) * a.lda;
    float4 lo[KS], hi[KS];
    float m = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k0 = ks * 32 + lg * 8;
      const bool ok = ar != nullptr && k0 < a.K;  // (K % 8 == 0: a group of eight is whole or absent)
      lo[ks] = ok ? nn_ld4(ar + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
      hi[ks] = ok ? nn_ld4(ar + k0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      m = fmaxf(m, fmaxf(fmaxf(fabsf(lo[ks].x), fabsf(lo[ks].y)), fmaxf(fabsf(lo[ks].z), fabsf(lo[ks].w))));
      m = fmaxf(m, fmaxf(fmaxf(fabsf(hi[ks].x), fabsf(hi[ks].y)), fmaxf(fabsf(hi[ks].z), fabsf(hi[ks].w))));
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));  // the row's four lane groups
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    rsh[rt] = amax_shift(__float_as_uint(m));
    const float sc = pow2f(rsh[rt]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 hh, ll;
      split2h8(lo[ks], hi[ks], sc, hh, ll);
      ah[rt][ks] = __builtin_bit_cast(f16x8, hh);
      al[rt][ks] = __builtin_bit_cast(f16x8, ll);
    }
  }
  // the accumulators' layout: row block rt, rows 16 rt + 4 lg + r, column 16 nt + lr
  float usc[2][4];  // 2^-(row shift) 2^-(W2 shift), applied as the rows leave
  const float uw = pow2f(-amax_shift(*a.amax_w));
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) usc[rt][r] = pow2f(-__shfl(rsh[rt], 4 * lg + r, 64)) * uw;
  f32x4 acc[2][4];
  float zc[2][4][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (BWD) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t s = e0 + wave * 32 + rt * 16 + 4 * lg + r;
          zc[rt][nt][r] = (s < a.E && nt < ntc) ? a.z[s * a.ldz + (nt0 + nt) * 16 + lr] : 0.f;
        }
      }
    }

  u32x4 pre[NL];  // the next panel in flight (PV % 256 == 0 but for KS = 1: half the threads)
  auto fetch = [&](int i, int nt) {
    const uint4* p = a.img + ((int64_t)i * a.NT + nt0 + nt) * PV;
#pragma unroll
    for (int l = 0; l < NL; ++l)
      if (KS > 1 || tid < PV) pre[l] = __builtin_bit_cast(u32x4, p[tid + 256 * l]);
  };
  auto park = [&](int slot) {
#pragma unroll
    for (int l = 0; l < NL; ++l)
      if (KS > 1 || tid < PV) ring[slot * PV + tid + 256 * l] = __builtin_bit_cast(uint4, pre[l]);
  };
  fetch(0, 0);
  park(0);
  int buf = 0;
  for (int i = 0; i < D; ++i) {
    if (i % kNnIc == 0) {
      // (every wave is past the previous panel's barrier: the last chunk's reads are done)
      for (int idx = tid; idx < kNnTile * (kNnIc / 4); idx += 256) {
        const int r = idx >> 2, c = 4 * (idx & 3);
        const int64_t s = e0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < a.E) v = nn_ld4(a.h + (int64_t)a.src[s] * a.ldh + i + c);
        nn_st4(hs + r * kNnHs + c, v);
      }
      __syncthreads();  // (also publishes panel (0, 0) before the first read)
    }
    float hv[2][4], dot[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        hv[rt][r] = hs[(wave * 32 + rt * 16 + 4 * lg + r) * kNnHs + (i % kNnIc)];
        dot[rt][r] = 0.f;
      }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (nt < ntc) {  // (uniform over the workgroup)
        const bool last = i == D - 1 && nt == ntc - 1;
        if (!last) fetch(nt + 1 < ntc ? i : i + 1, nt + 1 < ntc ? nt + 1 : 0);
        const uint4* pb = ring + buf * PV;
        f32x4 c[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const f16x8 bh = __builtin_bit_cast(f16x8, pb[(2 * ks) * 64 + lane]);
          const f16x8 bl = __builtin_bit_cast(f16x8, pb[(2 * ks + 1) * 64 + lane]);
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            c[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rt][ks], bh, c[rt], 0, 0, 0);
            c[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt][ks], bl, c[rt], 0, 0, 0);
            c[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt][ks], bh, c[rt], 0, 0, 0);
          }
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            acc[rt][nt][r] = __fmaf_rn(hv[rt][r], c[rt][r], acc[rt][nt][r]);
            if constexpr (BWD) dot[rt][r] = __fmaf_rn(zc[rt][nt][r], c[rt][r], dot[rt][r]);
          }
        if (!last) park(buf ^ 1);
        __syncthreads();
        buf ^= 1;
      }
    }
    if constexpr (BWD) {  // dh[e][i] of this column group: the 16 lanes of a row, a fixed butterfly
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float d = dot[rt][r];
#pragma unroll
          for (int o = 8; o >= 1; o >>= 1) d = __fadd_rn(d, __shfl_xor(d, o, 64));
          const int64_t s = e0 + wave * 32 + rt * 16 + 4 * lg + r;
          if (lr == 0 && s < a.E) a.dh[((int64_t)blockIdx.y * a.E + s) * D + i] = d * usc[rt][r];
        }
    }
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t s = e0 + wave * 32 + rt * 16 + 4 * lg + r;
      if (s >= a.E) continue;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (nt >= ntc) continue;
        float* p = a.out + s * a.ldo + (nt0 + nt) * 16 + lr;
        const float v = acc[rt][nt][r] * usc[rt][r];
        *p = (BWD && a.accumulate) ? __fadd_rn(*p, v) : v;
      }
    }
}

// out[v][c] = bias[c] + sum over v's CSR row t (ascending, from 0) and the G slabs (ascending) of
// X[g][idx ? idx[t] : t][c]: one thread per float4.  The forward's destination sum (in-CSR, idx
// NULL, one slab) and the backward's source sum of the dh partials (out-CSR, idx = out_inslot).
__global__ void __launch_bounds__(256)
nnconv_rows_sum_kernel(int64_t N, int D, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ idx,
                       const float* __restrict__ X, int64_t ldx, int G, int64_t slab,
                       const float* __restrict__ bias, float* __restrict__ out, int64_t ldo) {
  const int q = D / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * q) return;
  const int64_t v = t / q;
  const int c = 4 * (int)(t - v * q);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int e = rowptr[v]; e < rowptr[v + 1]; ++e) {
    const int64_t row = idx ? idx[e] : e;
    for (int g = 0; g < G; ++g) {
      const float4 x = nn_ld4(X + g * slab + row * ldx + c);
      s = make_float4(__fadd_rn(s.x, x.x), __fadd_rn(s.y, x.y), __fadd_rn(s.z, x.z), __fadd_rn(s.w, x.w));
    }
  }
  if (bias) {
    const float4 b = nn_ld4(bias + c);
    s = make_float4(__fadd_rn(s.x, b.x), __fadd_rn(s.y, b.y), __fadd_rn(s.z, b.z), __fadd_rn(s.w, b.w));
  }
  nn_st4(out + v * ldo + c, s);
}

// Partial dW2 of row block i over the edge range blockIdx.y: part[y][(i D + o) H + k].
__global__ void __launch_bounds__(256)
nnconv_wgrad_kernel(int64_t E, int64_t per, const int32_t* __restrict__ slot_dst, const int32_t* __restrict__ src,
                    const float* __restrict__ h, int64_t ldh, int D, const float* __restrict__ z, int64_t ldz,
                    int H, const float* __restrict__ g, int64_t ldg, float* __restrict__ part) {
  extern __shared__ float sm[];
  const int PD = nn_pitch(D), PH = nn_pitch(H);
  float* gs = sm;                    // [32][PD] dM rows
  float* zs = sm + kNnWgE * PD;      // [32][PH] z rows
  float* hcol = zs + kNnWgE * PH;    // [32] h[src][i]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int i = blockIdx.x;
  const int MT = D / 16, NT = H / 16;
  const int64_t e_beg = (int64_t)blockIdx.y * per, e_end = min(E, e_beg + per);
  f32x4 acc[8][4];
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t c0 = e_beg; c0 < e_end; c0 += kNnWgE) {
    __syncthreads();  // the previous chunk's reads are done
    for (int idx = tid; idx < kNnWgE * (D / 4); idx += 256) {
      const int r = idx / (D / 4), c = 4 * (idx - r * (D / 4));
      const int64_t s = c0 + r;
      nn_st4(gs + r * PD + c, s < e_end ? nn_ld4(g + (int64_t)slot_dst[s] * ldg + c) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    for (int idx = tid; idx < kNnWgE * (H / 4); idx += 256) {
      const int r = idx / (H / 4), c = 4 * (idx - r * (H / 4));
      const int64_t s = c0 + r;
      nn_st4(zs + r * PH + c, s < e_end ? nn_ld4(z + s * ldz + c) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    if (tid < kNnWgE) hcol[tid] = c0 + tid < e_end ? h[(int64_t)src[c0 + tid] * ldh + i] : 0.f;
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < kNnWgE / 4; ++ks) {
      const int e = 4 * ks + lg;  // A: row o = 16 mt + lr, k = e; B: column k = 16 nt + lr, k = e
      const float hv = hcol[e];
      float av[8];
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) av[mt] = mt < MT ? __fmul_rn(hv, gs[e * PD + 16 * mt + lr]) : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int nt = wave + 4 * j;
        if (nt < NT) {  // (uniform over the wave)
          const float bv = zs[e * PH + 16 * nt + lr];
#pragma unroll
          for (int mt = 0; mt < 8; ++mt)
            if (mt < MT) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv, acc[mt][j], 0, 0, 0);
        }
      }
    }
  }
  float* pp = part + (int64_t)blockIdx.y * D * D * H + (int64_t)i * D * H;
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nt = wave + 4 * j;
      if (mt < MT && nt < NT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) pp[(int64_t)(16 * mt + 4 * lg + r) * H + 16 * nt + lr] = acc[mt][j][r];
      }
    }
}

int check_nnconv(const char* who, int D, int H) {
  MVML_REQUIRE(D >= 16 && D <= 128 && D % 16 == 0, "%s: node width must be a multiple of 16 in [16, 128] (got %d)", who, D);
  MVML_REQUIRE(H >= 16 && H <= 256 && H % 16 == 0, "%s: edge hidden width must be a multiple of 16 in [16, 256] (got %d)", who, H);
  return MVML_OK;
}
bool edges_ok(int64_t E) { return E >= 0 && E < (int64_t(1) << 31) - kNnTile; }

size_t image_f_vec(int D, int H) { return (size_t)D * (D / 16) * nn_ks(H) * 128; }
size_t image_b_vec(int D, int H) { return (size_t)D * (H / 16) * nn_ks(D) * 128; }
struct NnImage {
  const uint32_t* amax;
  const uint4 *f, *b;
  NnImage(const void* p, int D, int H)
      : amax(static_cast<const uint32_t*>(p)), f(reinterpret_cast<const uint4*>(static_cast<const char*>(p) + 256)),
        b(f + image_f_vec(D, H)) {}
};

template <bool BWD>
int launch_tile(const NnTileArgs& a, int K, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.E, kNnTile), (unsigned)ceil_div(a.NT, 4));
  switch_const<1, 2, 4, 8>(nn_ks(K), [&](auto s) {
    nnconv_tile_kernel<decltype(s)::value, BWD><<<grid, 256, 0, st>>>(a);
    return MVML_OK;
  });
  return check_launch(BWD ? "nnconv_tile_kernel (backward)" : "nnconv_tile_kernel (forward)");
}

int wgrad_splits(int64_t E, int D) {
  const int64_t chunks = ceil_div(E, kNnWgE);
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(chunks, ceil_div(512, D)), 32));
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" size_t mvml_nnconv_image_bytes(int D, int H) {
  if (D < 16 || D > 128 || D % 16 || H < 16 || H > 256 || H % 16) return 0;
  return 256 + 16 * (image_f_vec(D, H) + image_b_vec(D, H));
}

extern "C" int mvml_nnconv_split_w2(int D, int H, const float* W2, void* image, void* stream) {
  clear_error();
  if (int rc = check_nnconv("nnconv_split_w2", D, H)) return rc;
  MVML_REQUIRE(W2 != nullptr && image != nullptr && aligned16(image), "nnconv_split_w2: W2 and a 16-byte aligned image are required");
  const hipStream_t st = as_stream(stream);
  if (int rc = absmax_launch((int64_t)D * D, H, W2, H, static_cast<uint32_t*>(image), false, st)) return rc;
  NnImage im(image, D, H);
  const int64_t n = (int64_t)(image_f_vec(D, H) + image_b_vec(D, H)) / 2;
  nnconv_split_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(D, H, W2, im.amax, const_cast<uint4*>(im.f),
                                                                  const_cast<uint4*>(im.b));
  return check_launch("nnconv_split_kernel");
}

extern "C" int mvml_nnconv_slot_dst(int64_t num_nodes, const int32_t* in_rowptr, int32_t* slot_dst, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "nnconv_slot_dst: bad num_nodes %lld", (long long)num_nodes);
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(in_rowptr != nullptr, "nnconv_slot_dst: in_rowptr is required");
  nnconv_slot_dst_kernel<<<(unsigned)ceil_div(num_nodes, 256), 256, 0, as_stream(stream)>>>(num_nodes, in_rowptr, slot_dst);
  return check_launch("nnconv_slot_dst_kernel");
}

extern "C" size_t mvml_nnconv_fwd_workspace_size(int64_t num_edges, int D) {
  if (num_edges < 0 || D <= 0) return 0;
  return carve_size((size_t)std::max<int64_t>(num_edges, 1) * D * 4) + 256;
}

extern "C" int mvml_nnconv_fwd(int64_t num_nodes, int64_t num_edges, const int32_t* in_rowptr, const int32_t* in_src,
                               const float* h, int64_t ldh, int D, const float* z, int64_t ldz, int H,
                               const void* image, const float* bias, float* out, int64_t ldo, void* workspace,
                               size_t workspace_bytes, void* stream) {
  clear_error();
  if (int rc = check_nnconv("nnconv_fwd", D, H)) return rc;
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31) && edges_ok(num_edges), "nnconv_fwd: bad sizes %lld, %lld",
               (long long)num_nodes, (long long)num_edges);
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(row_ok(h, ldh, D) && row_ok(out, ldo, D) && in_rowptr != nullptr && aligned16(bias),
               "nnconv_fwd: h and out must be 16-byte aligned with pitches >= D that are multiples of 4; in_rowptr is "
               "required, bias 16-byte aligned");
  MVML_REQUIRE(num_edges == 0 || (row_ok(z, ldz, H) && in_src != nullptr && image != nullptr && aligned16(image)),
               "nnconv_fwd: with edges, z (16-byte aligned, pitch >= H, a multiple of 4), in_src and the image are required");
  const size_t need = mvml_nnconv_fwd_workspace_size(num_edges, D);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("nnconv_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  Carver cv(workspace, workspace_bytes);
  float* rows = cv.take<float>((size_t)std::max<int64_t>(num_edges, 1) * D);
  if (num_edges > 0) {
    NnImage im(image, D, H);
    NnTileArgs a{};
    a.E = num_edges; a.A = z; a.lda = ldz; a.row_id = nullptr; a.K = H; a.src = in_src; a.h = h; a.ldh = ldh; a.D = D;
    a.img = im.f; a.NT = D / 16; a.amax_w = im.amax; a.out = rows; a.ldo = D;
    if (int rc = launch_tile<false>(a, H, st)) return rc;
  }
  nnconv_rows_sum_kernel<<<(unsigned)ceil_div(num_nodes * (D / 4), 256), 256, 0, st>>>(
      num_nodes, D, in_rowptr, nullptr, rows, D, 1, 0, bias, out, ldo);
  return check_launch("nnconv_rows_sum_kernel");
}

extern "C" size_t mvml_nnconv_bwd_data_workspace_size(int64_t num_edges, int D, int H) {
  if (num_edges < 0 || D <= 0 || H <= 0) return 0;
  return carve_size((size_t)ceil_div(H, kNnCols) * std::max<int64_t>(num_edges, 1) * D * 4) + 256;
}

extern "C" int mvml_nnconv_bwd_data(int64_t num_nodes, int64_t num_edges, const int32_t* in_src, const int32_t* slot_dst,
                                    const int32_t* out_rowptr, const int32_t* out_inslot, const float* h, int64_t ldh,
                                    int D, const float* z, int64_t ldz, int H, const void* image, const float* g_out,
                                    int64_t ldg, int accumulate, float* dz, int64_t lddz, float* dH, int64_t lddh,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (int rc = check_nnconv("nnconv_bwd_data", D, H)) return rc;
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31) && edges_ok(num_edges), "nnconv_bwd_data: bad sizes %lld, %lld",
               (long long)num_nodes, (long long)num_edges);
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(row_ok(h, ldh, D) && row_ok(g_out, ldg, D) && row_ok(dH, lddh, D) && out_rowptr != nullptr,
               "nnconv_bwd_data: h, g_out and dH must be 16-byte aligned with pitches >= D that are multiples of 4; "
               "out_rowptr is required");
  MVML_REQUIRE(num_edges == 0 || (row_ok(z, ldz, H) && row_ok(dz, lddz, H) && in_src != nullptr && slot_dst != nullptr &&
                                  out_inslot != nullptr && image != nullptr && aligned16(image)),
               "nnconv_bwd_data: with edges, z and dz (16-byte aligned, pitches >= H, multiples of 4), in_src, slot_dst, "
               "out_inslot and the image are required");
  const size_t need = mvml_nnconv_bwd_data_workspace_size(num_edges, D, H);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("nnconv_bwd_data: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  const int G = (int)ceil_div(H, kNnCols);
  Carver cv(workspace, workspace_bytes);
  float* dh = cv.take<float>((size_t)G * std::max<int64_t>(num_edges, 1) * D);
  if (num_edges > 0) {
    NnImage im(image, D, H);
    NnTileArgs a{};
    a.E = num_edges; a.A = g_out; a.lda = ldg; a.row_id = slot_dst; a.K = D; a.src = in_src; a.h = h; a.ldh = ldh; a.D = D;
    a.img = im.b; a.NT = H / 16; a.amax_w = im.amax; a.out = dz; a.ldo = lddz; a.accumulate = accumulate;
    a.z = z; a.ldz = ldz; a.dh = dh;
    if (int rc = launch_tile<true>(a, D, st)) return rc;
  }
  nnconv_rows_sum_kernel<<<(unsigned)ceil_div(num_nodes * (D / 4), 256), 256, 0, st>>>(
      num_nodes, D, out_rowptr, out_inslot, dh, D, G, num_edges * (int64_t)D, nullptr, dH, lddh);
  return check_launch("nnconv_rows_sum_kernel");
}

extern "C" size_t mvml_nnconv_bwd_weight_workspace_size(int64_t num_edges, int D, int H) {
  if (num_edges < 0 || D <= 0 || H <= 0) return 0;
  return carve_size((size_t)wgrad_splits(num_edges, D) * D * D * H * 4) + 256;
}

extern "C" int mvml_nnconv_bwd_weight(int64_t num_edges, const int32_t* in_src, const int32_t* slot_dst, const float* h,
                                      int64_t ldh, int D, const float* z, int64_t ldz, int H, const float* g_out,
                                      int64_t ldg, int accumulate, float* dW2, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  clear_error();
  if (int rc = check_nnconv("nnconv_bwd_weight", D, H)) return rc;
  MVML_REQUIRE(edges_ok(num_edges), "nnconv_bwd_weight: bad num_edges %lld", (long long)num_edges);
  MVML_REQUIRE(dW2 != nullptr && aligned16(dW2), "nnconv_bwd_weight: a 16-byte aligned dW2 is required");
  const int64_t n = (int64_t)D * D * H;
  if (num_edges == 0) return accumulate ? MVML_OK : mvml_fill_zero(dW2, 1, n * 4, n * 4, stream);
  MVML_REQUIRE(row_ok(h, ldh, D) && row_ok(g_out, ldg, D) && row_ok(z, ldz, H) && in_src != nullptr && slot_dst != nullptr,
               "nnconv_bwd_weight: h, g_out (pitches >= D) and z (pitch >= H) must be 16-byte aligned with pitches that "
               "are multiples of 4; in_src and slot_dst are required");
  const size_t need = mvml_nnconv_bwd_weight_workspace_size(num_edges, D, H);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("nnconv_bwd_weight: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  const int S = wgrad_splits(num_edges, D);
  const int64_t per = ceil_div(ceil_div(num_edges, kNnWgE), S) * kNnWgE;
  Carver cv(workspace, workspace_bytes);
  float* part = cv.take<float>((size_t)S * n);
  const size_t lds = (size_t)(kNnWgE * (nn_pitch(D) + nn_pitch(H)) + kNnWgE) * 4;
  nnconv_wgrad_kernel<<<dim3((unsigned)D, (unsigned)S), 256, lds, st>>>(num_edges, per, slot_dst, in_src, h, ldh, D, z, ldz,
                                                                        H, g_out, ldg, part);
  if (int rc = check_launch("nnconv_wgrad_kernel")) return rc;
  return colsum_final_launch(n, S, part, n, 1.f, accumulate ? 1.f : 0.f, dW2, st, "nnconv_bwd_weight (partial sum)");
}
