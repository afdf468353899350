// GAT aggregation backward, without float atomics (row layout and residual kinds:
// gat_agg_common.h; the forward it differentiates: gat_agg_fwd.hip).
//
// Backward (two passes, no float atomics):
//   A (per dst v):  g_a_e = <Z[src_e], g_rst[v]>_f per head; g_s = a*(g_a - sum_v a*g_a);
//                   g_pre = g_s * leaky'(s_e); d er[v] = sum_e g_pre; dR[v] = g_rst[v] (or
//                   g_out[v] for the head-mean residual)                 -> gpre_ws, gelr, gY
//   B (per src u):  dZ[u] = sum_{e: u->w} a_e * g_rst[w] + d el[u] attn_l + d er[u] attn_r,
//                   d el[u] = sum_{e: u->w} g_pre_e (gather over the out-CSR; out_inslot maps an
//                   out-edge to its in-CSR slot; g_rst[w] rows come back from gY's dR block)
//   dL/dattn_{l,r} = sum_n d{el,er}[n,h] Z[n,h,:]   (mvml_gat_attn_grad, gat_params.hip)
#include "gat_agg_common.h"

namespace mvml {
namespace {

constexpr int kWavesPerBlock = 4;  // the per-atom pair: one wave per atom

// Backward contract (mvml_gat_agg_bwd): gY[n] = [dZ_agg | dR | d el | d er] where dZ_agg is
// dL/dZ through update_all(u_mul_e, sum) only; the el / er paths of dL/dZ (d el x attn_l +
// d er x attn_r) are NOT added to it: the projection backward takes them exactly through two
// extra GEMM rows / columns (A_l = attn_l . W_fc, see mvml_gat_fold_attn_rows), which keeps
// the backward to ONE pass over Z and dZ.
//
// The molecule case (group of <= kWinL atoms and <= kECap in-edges) is one workgroup per node
// group: the group's CSR, out-CSR and attention are staged in LDS, then the columns are swept
// CW at a time with Z and g_rst (= dL/d rst from g_out, ELU' or 1/H) staged in LDS:
//   * thread per in-edge e: g_a[e,h] += <Z[src_e], g_rst[dst_e]> over the chunk's columns;
//   * CW/4 lanes per source atom u: dZ_agg[u] = sum over u's out-edges of a_e g_rst[dst_e];
//   * dR (g_rst, or g_out for the head-mean residual) is written from the staged rows;
// then the softmax backward runs in LDS (g_s = a (g_a - sum a g_a), g_pre = g_s leaky') and
// d er / d el are its per-destination / per-source sums.  Z, g_out and dZ cross HBM once.
// Every other group (large molecules, edge-heavy hubs) takes the per-atom dst / src pair.
constexpr int kBwdWaves = 4;  // LDS kernel: waves per SIMD its register budget allows
// Backward LDS layout: Z and g_rst chunks of the group's rows, 16-B slot c of row r at
// r*LPD + (c ^ bwd_sw<LPD>(r)): 128-B rows (LPD = 8) are XOR-swizzled so whole-row reads of
// different atoms spread over the banks; 256-B rows (LPD = 16) already span all 64 banks.
template <int LPD>
__device__ __forceinline__ int bwd_sw(int r) { return LPD == 8 ? (r >> 1) & 7 : 0; }  // 4, 16: none

// DPP move within a row of 16 lanes (bound_ctrl: sources outside the row read 0).
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// Sum over each aligned group of LPD (4, 8 or 16) lanes; valid in the group's last four lanes.
template <int LPD>
__device__ __forceinline__ float grp_sum_hi(float v) {
  v += dppf<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dppf<0x4E>(v);   // quad_perm [2,3,0,1]
  if (LPD >= 8) v += dppf<0x114>(v);  // row_shr:4
  if (LPD == 16) v += dppf<0x118>(v);  // row_shr:8
  return v;
}

// Chunk loop of the backward LDS kernel for a group of at most NPA * 64 atoms: 8 lanes per row
// (CW = 32 columns), NPA rows per lane octet.  The chunk rows (Z, g_out, and for ELU' the
// forward output) stream through a register ring (k+1 and k+2 in flight while chunk k is
// processed from LDS; k+1 only for two-pass groups).  Loads are unconditional (rows past the group read 0 through
// the buffer resource's range check; chunks past the end use an out-of-range offset), so the
// loop is straight-line and the vmcnt waits are exact; stores of rows past the group are
// skipped.
// Per chunk, the octet of destination atom d also forms g_a[e, h] += <Z[src_e], g_rst[d]> over
// the chunk's columns for d's in-edges: lane q dots its 16-B slice of the source row (LDS) with
// its slice of g_rst[d], a DPP octet sum finishes the dot, and one lane per edge adds it to
// s_ga (zeroed by the caller; every (edge, head) has exactly one writer).  That reads each
// source row slice once per in-edge: half the LDS bytes of an edge-per-thread dot.
// BIG: the out-CSR (s_odst / s_oslot) is read from global memory (g_odst / g_oslot, group
// edge base e0, first atom a0) instead of LDS, which the big window needs for its rows.
// SEP (mvml_gat_agg_bwd_res): dR goes to its own rows (resource rR, row pitch ldri floats; an
// empty resource when it is not formed: the stores are dropped) and stays out of the |max|
// bookkeeping, which then covers gY's columns only.
template <int H, int MODE, int NPA, int CW, int NT = 16 * CW, int WIN = kWinL, int ECAP = kECap,
          bool BIG = false, bool SEP = false>
__device__ __forceinline__ float bwd_lds_chunks(
    float4* zs, float4* gs, const float* s_att, const int* s_odst, const int* s_oslot,
    const int* s_orp, const int* s_rp, const uint16_t* s_src, float* s_ga,
    __amdgpu_buffer_rsrc_t rY, int ldyi, __amdgpu_buffer_rsrc_t rGo, __amdgpu_buffer_rsrc_t rO,
    __amdgpu_buffer_rsrc_t rG, int ldgi, int nr, int F, const int32_t* __restrict__ g_odst = nullptr,
    const int32_t* __restrict__ g_oslot = nullptr, int e0 = 0, int a0 = 0,
    const uint32_t* s_segI = nullptr, int nsegI = 0, const uint32_t* s_segO = nullptr,
    int nsegO = 0, const int* s_rs = nullptr, float4* s_part = nullptr,
    const uint32_t* s_oxe = nullptr, const uint16_t* s_oxb = nullptr, float* s_rmx = nullptr,
    __amdgpu_buffer_rsrc_t rR = __amdgpu_buffer_rsrc_t(), int ldri = 0) {
  static_assert(kEC == 5, "in-edge writer lanes assume 5 cached in-edges");
  constexpr int LPD = CW / 4, DPP = NT / LPD;
  auto odst = [&](int o) -> int { if constexpr (BIG) return g_odst[e0 + o] - a0; else return s_odst[o]; };
  auto oslot = [&](int o) -> int { if constexpr (BIG) return g_oslot[e0 + o] - e0; else return s_oslot[o]; };
  const int tid = threadIdx.x, ds = tid / LPD, q = tid % LPD;
  const int HF = H * F, nfc = F / CW, nch = H * nfc;
  const int ocols = MODE == 1 ? F : HF;
  // row byte offsets (recomputed where used: registers are the constraint at NPA = 2)
  auto yrow = [&](int p) { return 4u * (uint32_t)((ds + DPP * p) * ldyi); };
  auto grow = [&](int p) { return 4u * (uint32_t)((ds + DPP * p) * ldgi); };
  auto gorow = [&](int p) { return 4u * (uint32_t)((ds + DPP * p) * ocols); };
  auto orow = [&](int p) { return 4u * (uint32_t)((ds + DPP * p) * HF); };
  // "no access" offsets just past each resource (see fwd_lds_chunks): every load and store is
  // unconditional, so the compiler's vmcnt counts are exact
  const uint32_t noY = 4u * (uint32_t)(nr * ldyi), noGo = 4u * (uint32_t)(nr * ocols);
  const uint32_t noO = 4u * (uint32_t)(nr * HF), noG = 4u * (uint32_t)(nr * ldgi);
  auto rrow = [&](int p) { return 4u * (uint32_t)((ds + DPP * p) * ldri); };  // SEP: dR rows
  const uint32_t noR = 4u * (uint32_t)(nr * ldri);
  float gmx = 0.f;  // |max| of this thread's stores into gY (live rows, real chunks)
  float rmx[NPA];   // ... per row (s_rmx: the rows' |max| over dZ and dR, for per-row scales)
  bool live[NPA];
  // node role: the g_rst row slot (low 16 bits) and attention slot (high 16 bits) of the
  // first kEC out-edges of this octet's source atoms in registers (a missing edge reads the
  // atom's own row with a zero attention), so a chunk's gathers are independent LDS reads;
  // more out-edges (hubs) loop.
  static_assert(WIN * LPD <= 65536 && (ECAP + 1) * H <= 65536, "16-bit slots");
  uint32_t gsl[NPA][kEC];
  int ob[NPA], oend[NPA];
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    const int r = ds + DPP * p;
    live[p] = r < nr;
    rmx[p] = 0.f;
    ob[p] = live[p] ? s_orp[r] : 0;
    oend[p] = live[p] ? s_orp[r + 1] : 0;
#pragma unroll
    for (int i = 0; i < kEC; ++i) {
      const bool ok = ob[p] + i < oend[p];
      const int rr = ok ? odst(ob[p] + i) : r;
      gsl[p][i] = (uint32_t)(rr * LPD + (q ^ bwd_sw<LPD>(rr))) |
                  ((uint32_t)(ok ? oslot(ob[p] + i) * H : ECAP * H) << 16);
    }
  }
  // destination role: Z row slots of the first kEC in-edges (own row when missing; the dot is
  // then discarded), the in-edge base and in-degree
  uint32_t zsl[NPA][kEC];
  int ieb[NPA], ideg[NPA];
  // BIG: hub segments of this octet's rows — in-edges past kEC (segmented rows: none walked
  // here, bit 31) and out-edges past kEC (first | count << 12; their partials are added below)
  int rsg[NPA], oxb[NPA];
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    rsg[p] = 0;
    oxb[p] = 0xFFFF;
    if constexpr (BIG) {
      rsg[p] = live[p] ? s_rs[ds + DPP * p] : 0;
      oxb[p] = live[p] ? (int)s_oxb[ds + DPP * p] : 0xFFFF;
    }
  }
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    const int d = ds + DPP * p;
    ieb[p] = live[p] ? s_rp[d] : 0;
    ideg[p] = live[p] ? s_rp[d + 1] - ieb[p] : 0;
#pragma unroll
    for (int i = 0; i < kEC; ++i) {
      const int sr = i < ideg[p] ? s_src[ieb[p] + i] : d;
      zsl[p][i] = (uint32_t)(sr * LPD + (q ^ bwd_sw<LPD>(sr)));
    }
  }
  auto head_of = [&](int k) { return MODE == 1 ? k % H : k / nfc; };
  auto fch_of = [&](int k) { return MODE == 1 ? k / H : k % nfc; };
  auto col_of = [&](int k) { return head_of(k) * F + fch_of(k) * CW + 4 * q; };
  struct Rows { float4 z[NPA], g[NPA], o[NPA]; };
  // Mean mode: chunks are f-chunk-major (k = fc H + h), and g_rst = g_out / H is the same for
  // the H heads of an f-chunk, so g_out is loaded and gs staged only at h == 0 (the gs image of
  // chunk k stays valid for chunks k+1 .. k+H-1).
  auto load = [&](int k, Rows& R) {
    const bool ok = k < nch;
    const int col = col_of(k);
    const int gcol = MODE == 1 ? fch_of(k) * CW + 4 * q : col;
    const bool gload = MODE != 1 || head_of(k) == 0;  // uniform
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      R.z[p] = buf_ld4(rY, ok ? yrow(p) + 4u * (uint32_t)col : noY);
      if (gload) R.g[p] = buf_ld4(rGo, ok ? gorow(p) + 4u * (uint32_t)gcol : noGo);
      if (MODE == 0) R.o[p] = buf_ld4(rO, ok ? orow(p) + 4u * (uint32_t)col : noO);
    }
  };
  // stage chunk k: g_rst = g_out * ELU'(x) (ELU' = out + 1 for x <= 0, torch elu_backward on
  // the result) | g_out / H (head mean) | g_out; dR = g_rst, or g_out once per f-chunk (mean)
  auto stage = [&](int k, const Rows& R) {
    const bool ok = k < nch;
    const int h = head_of(k), fc = fch_of(k);
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      const int r = ds + DPP * p;
      float4 g = R.g[p];
      if (MODE == 0) {
        const float4 o = R.o[p];
        g.x *= o.x > 0.f ? 1.f : o.x + 1.f;
        g.y *= o.y > 0.f ? 1.f : o.y + 1.f;
        g.z *= o.z > 0.f ? 1.f : o.z + 1.f;
        g.w *= o.w > 0.f ? 1.f : o.w + 1.f;
      } else if (MODE == 1) {
        const float hh = (float)H;
        g = make_float4(g.x / hh, g.y / hh, g.z / hh, g.w / hh);
      }
      zs[r * LPD + (q ^ bwd_sw<LPD>(r))] = R.z[p];
      if (MODE != 1) {
        gs[r * LPD + (q ^ bwd_sw<LPD>(r))] = g;
        if constexpr (SEP) {
          buf_st4(rR, ok ? rrow(p) + 4u * (uint32_t)col_of(k) : noR, g);
        } else {
          buf_st4(rG, ok ? grow(p) + 4u * (uint32_t)(HF + col_of(k)) : noG, g);
          if (ok && r < nr) rmx[p] = amax4(rmx[p], g);
        }
      } else if (h == 0) {  // uniform branch: an all-out-of-range store is not free
        gs[r * LPD + (q ^ bwd_sw<LPD>(r))] = g;
        if constexpr (SEP) {
          buf_st4(rR, ok ? rrow(p) + 4u * (uint32_t)(fc * CW + 4 * q) : noR, R.g[p]);
        } else {
          buf_st4(rG, ok ? grow(p) + 4u * (uint32_t)(HF + fc * CW + 4 * q) : noG, R.g[p]);
          if (ok && r < nr) rmx[p] = amax4(rmx[p], R.g[p]);
        }
      }
    }
  };
  // chunks k+1 .. k+RB in flight (two-pass groups already move twice the bytes per chunk)
  constexpr int RB = NPA == 1 ? 2 : 1;
  Rows ring[RB];
  {
    Rows R0;
    load(0, R0);
#pragma unroll
    for (int i = 0; i < RB; ++i) load(1 + i, ring[i]);
    stage(0, R0);
  }
  __syncthreads();  // chunk 0
  for (int k = 0; k < nch; ++k) {
    const int h = head_of(k);
#pragma unroll
    for (int p = 0; p < NPA; ++p) {  // g_a partials of the in-edges of destination d
      const int d = ds + DPP * p;
      const float4 gd = gs[d * LPD + (q ^ bwd_sw<LPD>(d))];
      float t[kEC];
#pragma unroll
      for (int i = 0; i < kEC; ++i) t[i] = grp_sum_hi<LPD>(dot4(zs[zsl[p][i]], gd));
      if (q >= LPD - 4) {  // the group's last 4 lanes write in-edges 0..3, the first of them 4
        const int i0 = q - (LPD - 4);
        const float v = i0 == 0 ? t[0] : i0 == 1 ? t[1] : i0 == 2 ? t[2] : t[3];
        if (i0 < ideg[p]) s_ga[(ieb[p] + i0) * H + h] += v;
        if (i0 == 0 && ideg[p] > 4) s_ga[(ieb[p] + 4) * H + h] += t[4];
      }
      for (int i = kEC; i < (rsg[p] < 0 ? kEC : ideg[p]); ++i) {  // hubs (octet-uniform trip count)
        const int sr = s_src[ieb[p] + i];
        const float v = grp_sum_hi<LPD>(dot4(zs[sr * LPD + (q ^ bwd_sw<LPD>(sr))], gd));
        if (q == LPD - 4) s_ga[(ieb[p] + i) * H + h] += v;
      }
    }
    if constexpr (BIG) {  // hub in-edge segments: edge dots straight into s_ga (one writer each)
      for (int t = ds; t < nsegI; t += DPP) {
        const uint32_t sg = s_segI[t];
        const int d = (int)(sg >> 16), eb = (int)((sg >> 4) & 0xFFFu), c = (int)(sg & 15u) + 1;
        const float4 gd = gs[d * LPD + (q ^ bwd_sw<LPD>(d))];
        float v[kSegI];
#pragma unroll
        for (int j = 0; j < kSegI; ++j) {
          const int sr = s_src[eb + (j < c ? j : 0)];
          v[j] = grp_sum_hi<LPD>(dot4(zs[sr * LPD + (q ^ bwd_sw<LPD>(sr))], gd));
        }
        if (q >= LPD - 4) {  // lane i0 of the last four writes edges i0, i0 + 4
          const int i0 = q - (LPD - 4);
#pragma unroll
          for (int j = 0; j < kSegI; ++j)
            if (j % 4 == i0 && j < c) s_ga[(eb + j) * H + h] += v[j];
        }
      }
    }
    if constexpr (BIG) {  // hub out-edge segments: partial dZ sums to s_part
      for (int t = ds; t < nsegO; t += DPP) {
        const uint32_t sg = s_segO[t];
        const int c = (int)(sg & 15u) + 1;
        const uint32_t* oe = s_oxe + ((sg >> 4) & 0xFFFu);
        float4 part = f4(0.f);
        for (int j0 = 0; j0 < c; j0 += 4) {  // batches of 4 edges (registers)
          int od[4], sl[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t x = oe[j0 + j < c ? j0 + j : 0];
            od[j] = (int)(x >> 16);
            sl[j] = (int)(x & 0xFFFFu);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j)
            part = fma4(j0 + j < c ? s_att[sl[j] * H + h] : 0.f,
                        gs[od[j] * LPD + (q ^ bwd_sw<LPD>(od[j]))], part);
        }
        s_part[t * LPD + q] = part;
      }
    }
    float4 acc[NPA];  // dZ_agg of the source atoms over their out-edges
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      acc[p] = f4(0.f);
#pragma unroll
      for (int i = 0; i < kEC; ++i)
        acc[p] = fma4(s_att[(gsl[p][i] >> 16) + h], gs[gsl[p][i] & 0xFFFFu], acc[p]);
      for (int o = ob[p] + kEC; o < ((rsg[p] & 0xFFFFFF) ? ob[p] + kEC : oend[p]); ++o) {
        int od, sl;
        if (BIG && oxb[p] != 0xFFFF) {  // staged (hub partners: one or two edges past kEC)
          const uint32_t x = s_oxe[oxb[p] + o - ob[p] - kEC];
          od = (int)(x >> 16);
          sl = (int)(x & 0xFFFFu);
        } else {
          od = odst(o);
          sl = oslot(o);
        }
        acc[p] = fma4(s_att[sl * H + h], gs[od * LPD + (q ^ bwd_sw<LPD>(od))], acc[p]);
      }
    }
    __syncthreads();
    if constexpr (BIG) {  // this chunk's out-edge segment partials, in order
#pragma unroll
      for (int p = 0; p < NPA; ++p) {
        const int n = (rsg[p] >> 12) & 0xFFF, sb = rsg[p] & 0xFFF;
        for (int j = 0; j < n; ++j) acc[p] = add4(acc[p], s_part[(sb + j) * LPD + q]);
      }
    }
    stage(k + 1, ring[0]);
#pragma unroll
    for (int i = 0; i + 1 < RB; ++i) ring[i] = ring[i + 1];
    load(k + 1 + RB, ring[RB - 1]);
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      buf_st4(rG, grow(p) + 4u * (uint32_t)col_of(k), acc[p]);  // rows past the group: dropped
      if (ds + DPP * p < nr) rmx[p] = amax4(rmx[p], acc[p]);
    }
    __syncthreads();
  }
  // the rows' |max| over their LPD lanes (one writer per row; the caller adds d el / d er)
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    float m = rmx[p];
    gmx = fmaxf(gmx, m);
#pragma unroll
    for (int o = LPD / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (s_rmx && live[p] && q == 0) s_rmx[ds + DPP * p] = m;
  }
  return gmx;
}

// One workgroup of 512 threads per node group (2 per CU): the group's CSR, out-CSR and
// attention are staged in LDS, the column chunks stream through bwd_lds_chunks (one pass for
// groups of <= 64 atoms, two up to kWinL), then the softmax backward runs in LDS.
// BIG (kind bit 2): the big-window variant for the groups on the backward fallback list: 16-column
// chunks, 1024 threads (two passes of 256 rows), out-CSR and logits read from global memory
// (LDS holds the rows, the attention, the edge gradients and the in-CSR), one workgroup per CU
// walking the list.
template <int H, int MODE, int CW, int NT = 16 * CW, int WIN = kWinL, int ECAP = kECap, bool BIG = false,
          bool SEP = false>
__global__ void __launch_bounds__(NT, kBwdWaves)
gat_agg_bwd_lds_kernel(const int32_t* __restrict__ plan, int64_t G, const int32_t* __restrict__ rowptr,
                       const int32_t* __restrict__ in_src, const int32_t* __restrict__ out_rowptr,
                       const int32_t* __restrict__ out_dst, const int32_t* __restrict__ out_inslot,
                       const float* __restrict__ Y, int64_t ldy, int F, const float* __restrict__ elr,
                       const float* __restrict__ attn, const float* __restrict__ out,
                       const float* __restrict__ g_out, float slope, float* __restrict__ gY,
                       int64_t ldgy, int C, uint32_t* __restrict__ gy_amax,
                       uint32_t* __restrict__ gy_rows, float* __restrict__ gR = nullptr,
                       int64_t ldgr = 0) {
  constexpr int LPD = CW / 4;
  constexpr int DPP = NT / LPD;
  constexpr int NPM = WIN / DPP;  // passes over a full window
  static_assert(NPM * DPP == WIN && (NPM == 2 || NPM == 4), "the passes must tile the LDS rows exactly");
  __shared__ float4 zs[WIN * LPD];
  __shared__ float4 gs[WIN * LPD];
  __shared__ float s_att[(ECAP + 1) * H];  // + H zeros: the attention of a missing edge
  __shared__ float s_ga[ECAP * H];
  __shared__ uint16_t s_src[ECAP];
  __shared__ int s_odst[BIG ? 1 : ECAP], s_oslot[BIG ? 1 : ECAP];
  __shared__ int s_rp[WIN + 1], s_orp[WIN + 1];
  __shared__ float s_elr[BIG ? 1 : WIN * 2 * H];
  // BIG: hub segment tables (in-edges, out-edges), per-row segments, out-segment partials
  __shared__ uint32_t s_segI[BIG ? kSegCapI : 1], s_segO[BIG ? kSegCapO : 1];
  __shared__ int s_rs[BIG ? WIN : 1];
  __shared__ float4 s_part[BIG ? kSegCapO * LPD : 1];
  // out-edges past kEC of every row (dst row << 16 | in-slot), from row base s_oxb (0xFFFF:
  // past the table, read from global memory)
  __shared__ uint32_t s_oxe[BIG ? kOXCap : 1];
  __shared__ uint16_t s_oxb[BIG ? WIN : 1];
  __shared__ int s_wsum[BIG ? NT / 64 : 1];
  const GroupPlan gp(plan, G);
  const int nlist = BIG ? gp.count[1] : (int)blockIdx.x + 1;
  float gmx = 0.f;  // |max| of this thread's gY stores, committed once after the group loop
  for (int li = blockIdx.x; li < nlist; li += BIG ? gridDim.x : 1) {
  const int grp = BIG ? gp.bwd_list[li] : li;
  if (BIG) __syncthreads();  // the previous group's LDS reads are done
  if (!(gp.kind[grp] & (BIG ? 4 : 2))) continue;
  const int a0 = gp.start[grp], a1 = gp.start[grp + 1];
  const int tid = threadIdx.x;
  const int nr = a1 - a0, HF = H * F;
  const int ocols = MODE == 1 ? F : HF;
  const int e0 = rowptr[a0], ne = rowptr[a1] - e0;  // = the group's out-edge range too
  for (int i = tid; i <= nr; i += NT) {
    s_rp[i] = rowptr[a0 + i] - e0;
    s_orp[i] = out_rowptr[a0 + i] - e0;
  }
  for (int i = tid; i < ne; i += NT) {
    s_src[i] = (uint16_t)(in_src[e0 + i] - a0);
    if constexpr (!BIG) {
      s_odst[i] = out_dst[e0 + i] - a0;
      s_oslot[i] = out_inslot[e0 + i] - e0;
    }
  }
  for (int i = tid; i < ne * H; i += NT) s_att[i] = attn[(int64_t)e0 * H + i];
  if (tid < H) s_att[ECAP * H + tid] = 0.f;
  if constexpr (!BIG)
    for (int i = tid; i < nr * 2 * H; i += NT) s_elr[i] = elr[(int64_t)a0 * 2 * H + i];
  // BIG: after the chunk sweep the row buffers are free and hold the group's logits (zs) and
  // out-edge slots (gs) for the softmax backward and the d el sums
  float* s_elr_b = reinterpret_cast<float*>(zs);
  int* s_oslot_b = reinterpret_cast<int*>(gs);
  static_assert(!BIG || (WIN * 2 * H <= WIN * LPD * 4 && ECAP <= WIN * LPD * 4), "row buffers hold elr / slots");
  // gy_rows: the rows' |max| in the free row buffer after the sweep, past BIG's logits
  static_assert(WIN * 2 * H + WIN <= WIN * LPD * 4, "row buffer holds the logits and the row maxima");
  float* s_rmx = gy_rows ? reinterpret_cast<float*>(zs) + WIN * 2 * H : nullptr;
  auto elr_at = [&](int r, int c) -> float {  // elr of group row r, column c (el | er)
    if constexpr (BIG) return s_elr_b[r * 2 * H + c]; else return s_elr[r * 2 * H + c];
  };
  const int ldyi = (int)ldy, ldgi = (int)ldgy;
  const __amdgpu_buffer_rsrc_t rY = make_rsrc(Y + (int64_t)a0 * ldy, (uint32_t)(nr * ldyi) * 4u);
  const __amdgpu_buffer_rsrc_t rG = make_rsrc(gY + (int64_t)a0 * ldgy, (uint32_t)(nr * ldgi) * 4u);
  const __amdgpu_buffer_rsrc_t rGo = make_rsrc(g_out + (int64_t)a0 * ocols, (uint32_t)(nr * ocols) * 4u);
  const __amdgpu_buffer_rsrc_t rO = make_rsrc(out + (int64_t)a0 * HF, MODE == 0 ? (uint32_t)(nr * HF) * 4u : 0u);
  // SEP: the dR rows of the group (not formed: an empty range over gY, every store dropped)
  const int ldri = SEP && gR ? (int)ldgr : 0;
  const __amdgpu_buffer_rsrc_t rR =
      make_rsrc(SEP && gR ? gR + (int64_t)a0 * ldgr : gY, SEP && gR ? (uint32_t)(nr * ldri) * 4u : 0u);
  for (int i = tid; i < ne * H; i += NT) s_ga[i] = 0.f;
  __syncthreads();  // CSR / attention staged
  int nsegI = 0, nsegO = 0;
  if constexpr (BIG) {
    static_assert(NT >= WIN, "one row per thread for the segment scans");
    const bool lv = tid < nr;
    int rsI, rsO;
    nsegI = hub_segments<NT, kSegI, kSegCapI>(nr, lv ? s_rp[tid] : 0, lv ? s_rp[tid + 1] - s_rp[tid] : 0,
                                              s_segI, &rsI, s_wsum);
    const int ob = lv ? s_orp[tid] : 0, odeg = lv ? s_orp[tid + 1] - ob : 0;
    const int m = max(0, odeg - kEC);
    int mt;
    const int xb = block_excl_scan<NT>(m, s_wsum, &mt);
    const bool xok = xb + m <= kOXCap;
    for (int j = 0; j < (xok ? m : 0); ++j) {
      const int o = ob + kEC + j;
      s_oxe[xb + j] = (uint32_t)(out_dst[e0 + o] - a0) << 16 | (uint32_t)(out_inslot[e0 + o] - e0);
    }
    if (lv) s_oxb[tid] = (uint16_t)(xok && m ? xb : 0xFFFF);
    __syncthreads();  // s_wsum reads of the scan are done
    // out-edge segments index the table: "edge" e = xb + (out-edge - kEC)
    nsegO = hub_segments<NT, kSegO, kSegCapO, kSegMinO>(nr, xb - kEC, xok ? odeg : 0, s_segO, &rsO, s_wsum);
    if (lv) s_rs[tid] = rsO | (rsI ? (int)0x80000000 : 0);
    __syncthreads();
  }
  // (a macro, not a lambda: through a generic lambda every instance of this kernel compiled to
  // other machine code — DESIGN.md, "Aggregation source layout")
#define MVML_BWD_CHUNKS(NPA)                                                                       \
  gmx = fmaxf(gmx, bwd_lds_chunks<H, MODE, NPA, CW, NT, WIN, ECAP, BIG, SEP>(zs, gs, s_att, s_odst, s_oslot, s_orp, s_rp,  \
                                                       s_src, s_ga, rY, ldyi, rGo, rO, rG, ldgi, nr, F, \
                                                       out_dst, out_inslot, e0, a0, s_segI, nsegI, \
                                                       s_segO, nsegO, s_rs, s_part, s_oxe, s_oxb, s_rmx, rR, ldri))
  if (nr <= DPP) MVML_BWD_CHUNKS(1);
  else if (NPM == 2 || nr <= 2 * DPP) MVML_BWD_CHUNKS(2);
  else if (nr <= 3 * DPP) MVML_BWD_CHUNKS((NPM > 2 ? 3 : 2));
  else MVML_BWD_CHUNKS(NPM);
#undef MVML_BWD_CHUNKS
  __syncthreads();
  if constexpr (BIG) {
    for (int i = tid; i < nr * 2 * H; i += NT) s_elr_b[i] = elr[(int64_t)a0 * 2 * H + i];
    for (int i = tid; i < ne; i += NT) s_oslot_b[i] = out_inslot[e0 + i] - e0;
    __syncthreads();
  }
  // edge_softmax backward per (destination, head); g_pre replaces g_a in LDS
  for (int i = tid; i < nr * H; i += NT) {
    const int d = i / H, h = i % H;
    const int eb = s_rp[d], ee = s_rp[d + 1];
    const float er = elr_at(d, H + h);
    float dots = 0.f;
    for (int e = eb; e < ee; ++e) dots += s_att[e * H + h] * s_ga[e * H + h];
    float der = 0.f;
    for (int e = eb; e < ee; ++e) {
      const float g_s = s_att[e * H + h] * (s_ga[e * H + h] - dots);
      const float gp = (elr_at(s_src[e], h) + er) > 0.f ? g_s : g_s * slope;
      s_ga[e * H + h] = gp;
      der += gp;
    }
    gY[(int64_t)(a0 + d) * ldgy + C + H + h] = der;
    gmx = fmaxf(gmx, fabsf(der));
    if (s_rmx) atomicMax(reinterpret_cast<uint32_t*>(s_rmx) + d, __float_as_uint(fabsf(der)));
  }
  __syncthreads();
  for (int i = tid; i < nr * H; i += NT) {  // d el: sums over out-edges
    const int u = i / H, h = i % H;
    float del = 0.f;
    for (int o = s_orp[u]; o < s_orp[u + 1]; ++o) {
      int sl;
      if constexpr (BIG) sl = s_oslot_b[o]; else sl = s_oslot[o];
      del += s_ga[sl * H + h];
    }
    gY[(int64_t)(a0 + u) * ldgy + C + h] = del;
    gmx = fmaxf(gmx, fabsf(del));
    if (s_rmx) atomicMax(reinterpret_cast<uint32_t*>(s_rmx) + u, __float_as_uint(fabsf(del)));
  }
  if (s_rmx) {  // (LDS max of non-negative float bits: order-independent)
    __syncthreads();
    for (int r = tid; r < nr; r += NT) gy_rows[a0 + r] = __float_as_uint(s_rmx[r]);
  }
  }
  if (gy_amax) block_amax_commit<NT>(gmx, gy_amax);
}

// Pass A: one wave per destination v.
template <int H, int VPL>
__global__ void __launch_bounds__(kWavesPerBlock * 64)
gat_agg_bwd_dst_kernel(int64_t N, const int32_t* __restrict__ groups, int64_t G,
                       const int32_t* __restrict__ rowptr, const int32_t* __restrict__ in_src,
                       const float* __restrict__ Y, int64_t ldy, const float* __restrict__ elr,
                       const float* __restrict__ attn, const float* __restrict__ out,
                       const float* __restrict__ g_out, int F, float slope, int mode,
                       float* __restrict__ gpre, float* __restrict__ gY, int64_t ldgy,
                       float* __restrict__ gelr, int64_t ldgl, int skip_big,
                       uint32_t* __restrict__ gy_amax, uint32_t* __restrict__ gy_rows,
                       float* gR, int64_t ldgr, int ramax) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float gmx = 0.f;  // |max| of this thread's gY stores (block-uniform early returns only)
  // G > 0: one block per backward fallback group of the plan; G == 0: one wave per atom over
  // all atoms
  int64_t v, vend, vstep;
  if (G > 0) {
    const GroupPlan gp(groups, G);
    const int li = list_block(blockIdx.x, gridDim.x, gp.count[1]);
    if (li < 0) return;
    const int g = gp.bwd_list[li];
    if (skip_big && (gp.kind[g] & 4)) return;  // the big-window kernel takes it
    const int a0 = gp.start[g], a1 = gp.start[g + 1];
    v = a0 + wid;
    vend = a1;
    vstep = kWavesPerBlock;
  } else {
    v = xcd_block(blockIdx.x, gridDim.x) * kWavesPerBlock + wid;
    vend = min<int64_t>(v + 1, N);
    vstep = 1;
  }
  for (; v < vend; v += vstep) {
  const int HF = H * F;
  const int beg = rowptr[v], end = rowptr[v + 1];
  const int deg = end - beg;
  int hc[VPL];
  bool okc[VPL];
  float4 gr[VPL];
#pragma unroll
  for (int c = 0; c < VPL; ++c) {
    const int col = 4 * (lane + 64 * c);
    okc[c] = col < HF;
    hc[c] = okc[c] ? col / F : 0;
    gr[c] = okc[c] ? grst_of(g_out, out, v, col, HF, F, H, mode) : f4(0.f);
  }
  // dR[v]: per-head g_rst (flatten modes) or g_out (head-mean residual).  Written here so the
  // source pass can gather finished g_rst rows from gY instead of re-deriving them per edge.
  // gR: the dR rows (gY + H F with ldgr = ldgy in the projection-row layout; NULL: not formed);
  // ramax: whether they count in the |max| bookkeeping (they do where they are part of gY)
  float* grv = gR ? gR + v * ldgr : nullptr;
  float rmx = 0.f;  // this row's |max| (dR, d er) for gy_rows
#pragma unroll
  for (int c = 0; c < VPL; ++c) {
    const int col = 4 * (lane + 64 * c);
    if (mode != 1) {
      if (okc[c] && grv) {
        st4(grv + col, gr[c]);
        if (ramax) rmx = amax4(rmx, gr[c]);
      }
    } else if (col < F && grv) {
      const float4 go = ld4(g_out + v * F + col);
      st4(grv + col, go);
      if (ramax) rmx = amax4(rmx, go);
    }
  }
  float er[H];
#pragma unroll
  for (int h = 0; h < H; ++h) er[h] = elr[v * 2 * H + H + h];

  float dots[H];  // sum_e a_e * g_a_e per head
#pragma unroll
  for (int h = 0; h < H; ++h) dots[h] = 0.f;
  float ga_l[H], a_l[H];
  for (int base = 0; base < deg; base += 64) {
    const int cnt = min(64, deg - base);
    const int u_l = (base + lane < deg) ? in_src[beg + base + lane] : 0;
#pragma unroll
    for (int h = 0; h < H; ++h) ga_l[h] = 0.f;
    for (int j = 0; j < cnt; j += 2) {  // two source rows in flight
      const int j1 = min(j + 1, cnt - 1);
      const float* zu0 = Y + (int64_t)rl(u_l, j) * ldy;
      const float* zu1 = Y + (int64_t)rl(u_l, j1) * ldy;
      float4 z0[VPL], z1[VPL];
#pragma unroll
      for (int c = 0; c < VPL; ++c) {
        z0[c] = okc[c] ? ld4(zu0 + 4 * (lane + 64 * c)) : f4(0.f);
        z1[c] = okc[c] ? ld4(zu1 + 4 * (lane + 64 * c)) : f4(0.f);
      }
      float p0[H], p1[H];
#pragma unroll
      for (int h = 0; h < H; ++h) { p0[h] = 0.f; p1[h] = 0.f; }
#pragma unroll
      for (int c = 0; c < VPL; ++c)
        if (okc[c]) {
          add_at<H>(p0, hc[c], dot4(z0[c], gr[c]));
          add_at<H>(p1, hc[c], dot4(z1[c], gr[c]));
        }
      HeadReduce<H>::template all<false>(p0, lane);
      HeadReduce<H>::template all<false>(p1, lane);
#pragma unroll
      for (int h = 0; h < H; ++h) ga_l[h] = (lane == j) ? p0[h] : (lane == j1) ? p1[h] : ga_l[h];
    }
    const bool valid = base + lane < deg;
    float ag[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      a_l[h] = valid ? attn[(int64_t)(beg + base + lane) * H + h] : 0.f;
      ag[h] = a_l[h] * ga_l[h];
    }
    HeadReduce<H>::template all<false>(ag, lane);
#pragma unroll
    for (int h = 0; h < H; ++h) dots[h] += ag[h];
    if (deg > 64 && valid) {  // keep g_a for the second sweep
#pragma unroll
      for (int h = 0; h < H; ++h) gpre[(int64_t)(beg + base + lane) * H + h] = ga_l[h];
    }
  }
  float ger[H];
#pragma unroll
  for (int h = 0; h < H; ++h) ger[h] = 0.f;
  for (int base = 0; base < deg; base += 64) {
    const bool valid = base + lane < deg;
    const int64_t slot = beg + base + lane;
    float gp[H];
    if (valid) {
      const float* el_u = elr + (int64_t)in_src[slot] * 2 * H;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float a = (deg > 64) ? attn[slot * H + h] : a_l[h];
        const float ga = (deg > 64) ? gpre[slot * H + h] : ga_l[h];
        const float gs = a * (ga - dots[h]);
        gp[h] = (el_u[h] + er[h]) > 0.f ? gs : gs * slope;
        gpre[slot * H + h] = gp[h];
      }
    } else {
#pragma unroll
      for (int h = 0; h < H; ++h) gp[h] = 0.f;
    }
    HeadReduce<H>::template all<false>(gp, lane);
#pragma unroll
    for (int h = 0; h < H; ++h) ger[h] += gp[h];
  }
  store_heads<H>(gelr + v * ldgl + H, ger, lane);
#pragma unroll
  for (int h = 0; h < H; ++h) rmx = fmaxf(rmx, fabsf(ger[h]));
  gmx = fmaxf(gmx, rmx);
  if (gy_rows) {  // the first writer of the row's |max| (the source pass adds dZ, d el)
    rmx = wave_max(rmx);
    if (lane == 0) gy_rows[v] = __float_as_uint(rmx);
  }
  }
  if (gy_amax) block_amax_commit<kWavesPerBlock * 64>(gmx, gy_amax);
}

// Pass B: one wave per source u (out-CSR gather).
template <int H, int VPL>
__global__ void __launch_bounds__(kWavesPerBlock * 64)
gat_agg_bwd_src_kernel(int64_t N, const int32_t* __restrict__ groups, int64_t G,
                       const int32_t* __restrict__ rowptr, const int32_t* __restrict__ out_rowptr,
                       const int32_t* __restrict__ out_dst, const int32_t* __restrict__ out_inslot,
                       const float* __restrict__ attn, const float* __restrict__ gpre,
                       const float* __restrict__ out, const float* __restrict__ g_out, int F,
                       int mode, float* __restrict__ gY, int64_t ldgy, float* __restrict__ gelr,
                       int64_t ldgl, int skip_big, uint32_t* __restrict__ gy_amax,
                       uint32_t* __restrict__ gy_rows, const float* gR, int64_t ldgr) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float gmx = 0.f;  // |max| of this thread's gY stores (block-uniform early returns only)
  // G > 0: one block per backward fallback group of the plan; G == 0: one wave per atom over
  // all atoms
  int64_t u, vend, vstep;
  if (G > 0) {
    const GroupPlan gp(groups, G);
    const int li = list_block(blockIdx.x, gridDim.x, gp.count[1]);
    if (li < 0) return;
    const int g = gp.bwd_list[li];
    if (skip_big && (gp.kind[g] & 4)) return;  // the big-window kernel takes it
    const int a0 = gp.start[g], a1 = gp.start[g + 1];
    u = a0 + wid;
    vend = a1;
    vstep = kWavesPerBlock;
  } else {
    u = xcd_block(blockIdx.x, gridDim.x) * kWavesPerBlock + wid;
    vend = min<int64_t>(u + 1, N);
    vstep = 1;
  }
  for (; u < vend; u += vstep) {
  const int HF = H * F;
  const int beg = out_rowptr[u], end = out_rowptr[u + 1];
  const int deg = end - beg;
  int hc[VPL];
  bool okc[VPL];
  float4 gz[VPL];
#pragma unroll
  for (int c = 0; c < VPL; ++c) {
    const int col = 4 * (lane + 64 * c);
    okc[c] = col < HF;
    hc[c] = okc[c] ? col / F : 0;
    gz[c] = f4(0.f);
  }
  float gel[H];
#pragma unroll
  for (int h = 0; h < H; ++h) gel[h] = 0.f;
  for (int base = 0; base < deg; base += 64) {
    const int cnt = min(64, deg - base);
    int w_l = 0;
    float a_l[H], gp_l[H];
    if (base + lane < deg) {
      w_l = out_dst[beg + base + lane];
      const int64_t js = out_inslot[beg + base + lane];
#pragma unroll
      for (int h = 0; h < H; ++h) { a_l[h] = attn[js * H + h]; gp_l[h] = gpre[js * H + h]; }
    } else {
#pragma unroll
      for (int h = 0; h < H; ++h) { a_l[h] = 0.f; gp_l[h] = 0.f; }
    }
    HeadReduce<H>::template all<false>(gp_l, lane);
#pragma unroll
    for (int h = 0; h < H; ++h) gel[h] += gp_l[h];
    for (int j = 0; j < cnt; j += 2) {  // two g_rst rows in flight
      const int j1 = min(j + 1, cnt - 1);
      const bool two = j + 1 < cnt;  // (uniform)
      const int w0 = rl(w_l, j), w1 = rl(w_l, j1);
      float a0[H], a1[H];
#pragma unroll
      for (int h = 0; h < H; ++h) { a0[h] = rl(a_l[h], j); a1[h] = rl(a_l[h], j1); }
      // g_rst rows written by the dst pass (gR == NULL: dR is not formed, re-derived per edge)
      const bool derive = mode == 1 || !gR;
      const float* gw0 = gR + (int64_t)w0 * ldgr;
      const float* gw1 = gR + (int64_t)w1 * ldgr;
      float4 g0[VPL], g1[VPL];
#pragma unroll
      for (int c = 0; c < VPL; ++c) {
        const int col = 4 * (lane + 64 * c);
        g0[c] = !okc[c] ? f4(0.f) : derive ? grst_of(g_out, out, w0, col, HF, F, H, mode) : ld4(gw0 + col);
        g1[c] = !okc[c] ? f4(0.f) : derive ? grst_of(g_out, out, w1, col, HF, F, H, mode) : ld4(gw1 + col);
      }
#pragma unroll
      for (int c = 0; c < VPL; ++c)
        if (okc[c]) {
          gz[c] = fma4(pick<H>(a0, hc[c]), g0[c], gz[c]);
          if (two) gz[c] = fma4(pick<H>(a1, hc[c]), g1[c], gz[c]);
        }
    }
  }
  // dZ through the aggregation only; the el / er paths (d el x attn_l + d er x attn_r) reach
  // the projection's gradients through the [d el | d er] columns (mvml_gat_agg_bwd contract)
  float* gyu = gY + u * ldgy;
  float rmx = 0.f;
#pragma unroll
  for (int c = 0; c < VPL; ++c)
    if (okc[c]) {
      st4(gyu + 4 * (lane + 64 * c), gz[c]);
      rmx = amax4(rmx, gz[c]);
    }
  store_heads<H>(gelr + u * ldgl, gel, lane);
#pragma unroll
  for (int h = 0; h < H; ++h) rmx = fmaxf(rmx, fabsf(gel[h]));
  gmx = fmaxf(gmx, rmx);
  if (gy_rows) {  // the destination pass wrote this row's first part (stream order)
    rmx = wave_max(rmx);
    if (lane == 0) gy_rows[u] = max(gy_rows[u], __float_as_uint(rmx));
  }
  }
  if (gy_amax) block_amax_commit<kWavesPerBlock * 64>(gmx, gy_amax);
}

// ---- Head-mean layer backward by SOURCE atom (MVML_OPT_MEAN_SRC) -----------------------------
// In mean mode g_rst = g_out / H does not depend on the head, so both products of the backward
//   dZ[u, h, :] = sum_{e: u -> w} a_e,h g_out[w, :] / H          (update_all(u_mul_e, sum) backward)
//   g_a[e, h]   = <Z[u, h, :], g_out[w, :] / H>                   (the edge-weight gradient)
// are formed by the wave that owns SOURCE u: its projection row Z[u] (H F floats) is read once,
// straight from HBM into registers, and only the F-wide g_out rows of its out-neighbours are
// gathered (from the XCD's L2: xcd_block keeps neighbouring atoms on one XCD) — no LDS window,
// no chunk barriers, whatever the molecule size.  Lane l owns f-columns 4 (l + 64 j) of every
// head, so a g_out row is loaded once per edge (not once per head).  dZ walks the out-edges in
// out-CSR order with the atomwise pass's arithmetic (g_out / H, then fma), so it is bitwise
// the atomwise dZ; g_a is written per edge (one writer: the edge's source) for the softmax pass.
// (ld4nt / st4nt: the projection rows read once and the dZ rows written once pass through
// without displacing the g_out rows the XCD's waves share in L2)
template <int H, int NJ>
__global__ void __launch_bounds__(256)
gat_mean_bwd_src_kernel(int64_t N, const int32_t* __restrict__ out_rowptr,
                        const int32_t* __restrict__ out_dst, const int32_t* __restrict__ out_inslot,
                        const float* __restrict__ Y, int64_t ldy, const float* __restrict__ attn,
                        const float* __restrict__ g_out, int F, float* __restrict__ ga,
                        float* __restrict__ gY, int64_t ldgy, uint32_t* __restrict__ gy_amax,
                        uint32_t* __restrict__ gy_rows, float* gR, int64_t ldgr, int ramax) {
  const int lane = threadIdx.x & 63;
  const int64_t u = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float gmx = 0.f;
  if (u < N) {  // (no early return: block_amax_commit below has a barrier)
    const int nf4 = F / 4, HF = H * F;
    float* gru = gR ? gR + u * ldgr : nullptr;  // dR row (gat_agg_bwd_dst_kernel: gR / ramax)
    const float hh = (float)H;
    bool okj[NJ];
    float4 z[H][NJ], dz[H][NJ];
    const float* zu = Y + u * ldy;
    float* gyu = gY + u * ldgy;
    float rmx = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int fj = lane + 64 * j;
      okj[j] = fj < nf4;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        z[h][j] = okj[j] ? ld4nt(zu + h * F + 4 * fj) : f4(0.f);
        dz[h][j] = f4(0.f);
      }
      if (okj[j] && gru) {  // dR[u] = g_out[u] (the head-mean residual's gradient)
        const float4 go = ld4(g_out + u * F + 4 * fj);
        st4nt(gru + 4 * fj, go);
        if (ramax) rmx = amax4(rmx, go);
      }
    }
    const int ob = out_rowptr[u], oe = out_rowptr[u + 1];
    for (int base = ob; base < oe; base += 64) {
      const int cnt = min(64, oe - base);
      int w_l = 0, s_l = 0;
      float a_l[H];
#pragma unroll
      for (int h = 0; h < H; ++h) a_l[h] = 0.f;
      if (lane < cnt) {
        w_l = out_dst[base + lane];
        s_l = out_inslot[base + lane];
#pragma unroll
        for (int h = 0; h < H; ++h) a_l[h] = attn[(int64_t)s_l * H + h];
      }
      // two out-edges per trip: both g_out rows are loaded before either is used
      for (int j = 0; j < cnt; j += 2) {
        const int j1 = min(j + 1, cnt - 1);
        const bool two = j + 1 < cnt;  // (uniform)
        const float* gw0 = g_out + (int64_t)rl(w_l, j) * F;
        const float* gw1 = g_out + (int64_t)rl(w_l, j1) * F;
        float4 g0[NJ], g1[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
          g0[jj] = okj[jj] ? ld4(gw0 + 4 * (lane + 64 * jj)) : f4(0.f);
          g1[jj] = okj[jj] ? ld4(gw1 + 4 * (lane + 64 * jj)) : f4(0.f);
        }
        float a0[H], a1[H], p0[H], p1[H];
#pragma unroll
        for (int h = 0; h < H; ++h) { a0[h] = rl(a_l[h], j); a1[h] = rl(a_l[h], j1); p0[h] = 0.f; p1[h] = 0.f; }
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
          const float4 ga4 = make_float4(g0[jj].x / hh, g0[jj].y / hh, g0[jj].z / hh, g0[jj].w / hh);
          const float4 gb4 = make_float4(g1[jj].x / hh, g1[jj].y / hh, g1[jj].z / hh, g1[jj].w / hh);
#pragma unroll
          for (int h = 0; h < H; ++h) {
            dz[h][jj] = fma4(a0[h], ga4, dz[h][jj]);
            p0[h] += dot4(z[h][jj], ga4);
            if (two) dz[h][jj] = fma4(a1[h], gb4, dz[h][jj]);
            p1[h] += dot4(z[h][jj], gb4);
          }
        }
        HeadReduce<H>::template all<false>(p0, lane);
        store_heads<H>(ga + (int64_t)rl(s_l, j) * H, p0, lane);
        if (two) {
          HeadReduce<H>::template all<false>(p1, lane);
          store_heads<H>(ga + (int64_t)rl(s_l, j1) * H, p1, lane);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (okj[j]) {
#pragma unroll
        for (int h = 0; h < H; ++h) {
          st4nt(gyu + h * F + 4 * (lane + 64 * j), dz[h][j]);
          rmx = amax4(rmx, dz[h][j]);
        }
      }
    const float wm = wave_max(rmx);
    gmx = fmaxf(gmx, wm);
    if (gy_rows && lane == 0) gy_rows[u] = __float_as_uint(wm);  // the first writer of the row
  }
  if (gy_amax) block_amax_commit<256>(gmx, gy_amax);
}

// edge_softmax + LeakyReLU backward per destination v (thread per atom, the LDS kernel's
// arithmetic and edge order): g_a -> g_pre in place, d er[v] -> gY[v, C + H ..]
template <int H>
__global__ void __launch_bounds__(256)
gat_mean_bwd_softmax_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ in_src,
                            const float* __restrict__ elr, const float* __restrict__ attn, float slope,
                            float* __restrict__ gpre, float* __restrict__ gY, int64_t ldgy, int C) {
  const int64_t v = xcd_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (v >= N) return;
  const int eb = rowptr[v], ee = rowptr[v + 1];
  float er[H], dots[H], der[H];
#pragma unroll
  for (int h = 0; h < H; ++h) { er[h] = elr[v * 2 * H + H + h]; dots[h] = 0.f; der[h] = 0.f; }
  for (int e = eb; e < ee; ++e)
#pragma unroll
    for (int h = 0; h < H; ++h) dots[h] += attn[(int64_t)e * H + h] * gpre[(int64_t)e * H + h];
  for (int e = eb; e < ee; ++e) {
    const float* el = elr + (int64_t)in_src[e] * 2 * H;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float g_s = attn[(int64_t)e * H + h] * (gpre[(int64_t)e * H + h] - dots[h]);
      const float gp = (el[h] + er[h]) > 0.f ? g_s : g_s * slope;
      gpre[(int64_t)e * H + h] = gp;
      der[h] += gp;
    }
  }
#pragma unroll
  for (int h = 0; h < H; ++h) gY[v * ldgy + C + H + h] = der[h];
}

// d el[u] = sum over u's out-edges of g_pre (out-CSR order); the row |max| gains d el / d er.
template <int H>
__global__ void __launch_bounds__(256)
gat_mean_bwd_gel_kernel(int64_t N, const int32_t* __restrict__ out_rowptr,
                        const int32_t* __restrict__ out_inslot, const float* __restrict__ gpre,
                        float* __restrict__ gY, int64_t ldgy, int C, uint32_t* __restrict__ gy_amax,
                        uint32_t* __restrict__ gy_rows) {
  const int64_t u = xcd_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  float m = 0.f;
  if (u < N) {
    float g[H];
#pragma unroll
    for (int h = 0; h < H; ++h) g[h] = 0.f;
    for (int o = out_rowptr[u]; o < out_rowptr[u + 1]; ++o) {
      const float* p = gpre + (int64_t)out_inslot[o] * H;
#pragma unroll
      for (int h = 0; h < H; ++h) g[h] += p[h];
    }
    float* row = gY + u * ldgy + C;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      row[h] = g[h];
      m = fmaxf(m, fmaxf(fabsf(g[h]), fabsf(row[H + h])));
    }
    if (gy_rows) gy_rows[u] = max(gy_rows[u], __float_as_uint(m));
  }
  if (gy_amax) block_amax_commit<256>(m, gy_amax);
}

// ---- Flatten layer backward by source atom (MVML_OPT_FLAT_SRC), for large molecules ----------
// The flatten layer's g_rst (= g_out x ELU'(out)) is per head, so the source-owned form needs
// the g_rst rows of the out-neighbours.  One pass: the wave of source u forms its own g_rst row
// once from g_out[u] and out[u] (ELU'(x) = out + 1 below 0) and writes it as dR[u];
// for each out-edge u -> w it gathers the g_out[w] (and out[w]) rows — read by w's own wave and by
// w's other in-neighbours' waves at about the same time, so from the XCD's L2 — and forms g_rst[w]
// in registers with the same arithmetic, then dZ[u] += a_e g_rst[w] (out-CSR order) and
// g_a[e] = <Z[u], g_rst[w]> per head.  (Round 4 had a two-pass form — every g_rst row written
// first, then gathered — with the same bits; measured slower, deleted in round 5.)
template <int H, int NJ, int MODE, int U = 2>
__global__ void __launch_bounds__(256)
gat_flat_bwd_src1_kernel(int64_t N, const int32_t* __restrict__ out_rowptr,
                         const int32_t* __restrict__ out_dst, const int32_t* __restrict__ out_inslot,
                         const float* __restrict__ Y, int64_t ldy, const float* __restrict__ attn,
                         const float* __restrict__ out, const float* __restrict__ g_out, int F,
                         float* __restrict__ ga, float* __restrict__ gY, int64_t ldgy,
                         uint32_t* __restrict__ gy_amax, uint32_t* __restrict__ gy_rows,
                         float* gR, int64_t ldgr, int ramax) {
  const int lane = threadIdx.x & 63;
  const int64_t u = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float gmx = 0.f;
  if (u < N) {  // (no early return: block_amax_commit below has a barrier)
    const int HF = H * F;
    bool okc[NJ];
    int hc[NJ];
    float4 z[NJ], dz[NJ];
    float rmx = 0.f;
    auto grst = [&](int64_t w, int c) -> float4 {  // g_rst[w, 4 (lane + 64 c) ..]
      const int col = 4 * (lane + 64 * c);
      float4 g = ld4(g_out + w * HF + col);
      if (MODE == 0) {
        const float4 o = ld4(out + w * HF + col);
        g.x *= o.x > 0.f ? 1.f : o.x + 1.f;
        g.y *= o.y > 0.f ? 1.f : o.y + 1.f;
        g.z *= o.z > 0.f ? 1.f : o.z + 1.f;
        g.w *= o.w > 0.f ? 1.f : o.w + 1.f;
      }
      return g;
    };
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
      const int col = 4 * (lane + 64 * c);
      okc[c] = col < HF;
      hc[c] = okc[c] ? col / F : 0;
      z[c] = okc[c] ? ld4nt(Y + u * ldy + col) : f4(0.f);
      dz[c] = f4(0.f);
      if (okc[c] && gR) {  // dR[u] = g_rst[u] (gat_agg_bwd_dst_kernel: gR / ramax)
        const float4 g = grst(u, c);
        st4nt(gR + u * ldgr + col, g);
        if (ramax) rmx = amax4(rmx, g);
      }
    }
    const int ob = out_rowptr[u], oe = out_rowptr[u + 1];
    for (int base = ob; base < oe; base += 64) {
      const int cnt = min(64, oe - base);
      int w_l = 0, s_l = 0;
      float a_l[H];
#pragma unroll
      for (int h = 0; h < H; ++h) a_l[h] = 0.f;
      if (lane < cnt) {
        w_l = out_dst[base + lane];
        s_l = out_inslot[base + lane];
#pragma unroll
        for (int h = 0; h < H; ++h) a_l[h] = attn[(int64_t)s_l * H + h];
      }
      for (int j = 0; j < cnt; j += U) {  // U out-neighbours' rows in flight
        float4 g[U][NJ];
#pragma unroll
        for (int t = 0; t < U; ++t) {
          const int64_t wt = rl(w_l, min(j + t, cnt - 1));  // past the chunk: a duplicate row, unused
#pragma unroll
          for (int c = 0; c < NJ; ++c) g[t][c] = okc[c] ? grst(wt, c) : f4(0.f);
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
          if (j + t >= cnt) break;  // (uniform)
          float a[H], pd[H];
#pragma unroll
          for (int h = 0; h < H; ++h) { a[h] = rl(a_l[h], j + t); pd[h] = 0.f; }
#pragma unroll
          for (int c = 0; c < NJ; ++c)
            if (okc[c]) {
              dz[c] = fma4(pick<H>(a, hc[c]), g[t][c], dz[c]);
              add_at<H>(pd, hc[c], dot4(z[c], g[t][c]));
            }
          HeadReduce<H>::template all<false>(pd, lane);
          store_heads<H>(ga + (int64_t)rl(s_l, j + t) * H, pd, lane);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NJ; ++c)
      if (okc[c]) {
        st4nt(gY + u * ldgy + 4 * (lane + 64 * c), dz[c]);
        rmx = amax4(rmx, dz[c]);
      }
    const float wm = wave_max(rmx);
    gmx = fmaxf(gmx, wm);
    if (gy_rows && lane == 0) gy_rows[u] = __float_as_uint(wm);  // the first writer of the row
  }
  if (gy_amax) block_amax_commit<256>(gmx, gy_amax);
}

// ---------------------------------------------------------------------------------- dispatch
// One backward: what every kernel family reads.  gR / ldgr: the dR rows (gY + H F at gY's pitch
// in the projection-row layout; NULL: not formed); ramax: whether they count in the |max|
// bookkeeping (they do where they are part of gY).
struct BwdArgs {
  int64_t N;
  const int32_t* groups;
  int64_t G;
  const int32_t *rp, *src, *orp, *odst, *oslot;
  const float* Y;
  int64_t ldy;
  const float *elr, *attn, *out, *g_out;
  int F;
  float slope;
  int mode;
  float *gpre, *gY;
  int64_t ldgy;
  int C;
  uint32_t *gy_amax, *gy_rows;
  float* gR;
  int64_t ldgr;
  int ramax;
  hipStream_t st;
  // with per-row maxima requested, max |gY| comes from them at the end (no per-block atomics)
  uint32_t* blk_amax() const { return gy_rows ? nullptr : gy_amax; }
};

// The source-atom backwards' common end: the edge softmax backward per destination, d el per
// source, then max |gY| from the rows' maxima.
template <int H>
int finish_src_bwd(const BwdArgs& a) {
  const unsigned b256 = (unsigned)ceil_div(a.N, 256);
  gat_mean_bwd_softmax_kernel<H><<<b256, 256, 0, a.st>>>(a.N, a.rp, a.src, a.elr, a.attn, a.slope, a.gpre, a.gY,
                                                         a.ldgy, a.C);
  int rc = check_launch("gat_mean_bwd_softmax_kernel");
  if (rc) return rc;
  gat_mean_bwd_gel_kernel<H><<<b256, 256, 0, a.st>>>(a.N, a.orp, a.oslot, a.gpre, a.gY, a.ldgy, a.C, a.blk_amax(),
                                                     a.gy_rows);
  rc = check_launch("gat_mean_bwd_gel_kernel");
  if (rc) return rc;
  return launch_rows_amax(a.N, a.gy_rows, a.gy_amax, a.st);
}

// Flatten layer by source atom, one pass, one out-neighbour row per trip.
template <int H>
int launch_flat_src1(const BwdArgs& a) {
  const int rc = switch_const<1, 2, 3, 4, 5, 6, 7, 8>((int)ceil_div(H * a.F / 4, 64), [&](auto nj) {
    return switch_const<0, 2>(a.mode, [&](auto m) {
      gat_flat_bwd_src1_kernel<H, decltype(nj)::value, decltype(m)::value, 1>
          <<<(unsigned)ceil_div(a.N, 4), 256, 0, a.st>>>(a.N, a.orp, a.odst, a.oslot, a.Y, a.ldy, a.attn, a.out,
                                                         a.g_out, a.F, a.gpre, a.gY, a.ldgy, a.blk_amax(),
                                                         a.gy_rows, a.gR, a.ldgr, a.ramax);
      return check_launch("gat_flat_bwd_src1_kernel");
    });
  });
  if (rc == kNoCase) {
    set_error("gat_agg_bwd: flat-src path needs H F <= 2048");
    return MVML_ERR_INVALID;
  }
  return rc ? rc : finish_src_bwd<H>(a);
}

// Head-mean layer by source atom.  wide (mvml_gat_agg_bwd_res with dR apart from gY): F > 1024,
// which only H = 1 reaches, takes an 8-slot instance, so that this path holds every shape there.
template <int H>
int launch_mean_src(const BwdArgs& a, bool wide) {
  const int nj = (int)ceil_div(a.F / 4, 64);
  const int rc = switch_const<1, 2, 3, 4, 8>(nj <= 4 ? nj : wide ? 8 : 0, [&](auto s) {
    constexpr int NJ = decltype(s)::value;
    if constexpr (NJ == 8 && H != 1) return kNoCase;
    else {
      gat_mean_bwd_src_kernel<H, NJ><<<(unsigned)ceil_div(a.N, 4), 256, 0, a.st>>>(
          a.N, a.orp, a.odst, a.oslot, a.Y, a.ldy, a.attn, a.g_out, a.F, a.gpre, a.gY, a.ldgy, a.blk_amax(),
          a.gy_rows, a.gR, a.ldgr, a.ramax);
      return check_launch("gat_mean_bwd_src_kernel");
    }
  });
  if (rc == kNoCase) {
    set_error("gat_agg_bwd: mean-src path needs F <= 1024");
    return MVML_ERR_INVALID;
  }
  return rc ? rc : finish_src_bwd<H>(a);
}

// One LDS-window launch (the molecule window or the big one); gR / ldgr: the SEP instances' dR rows
template <typename Kernel>
void launch_lds_bwd(Kernel kernel, unsigned blocks, unsigned threads, const BwdArgs& a, float* gR, int64_t ldgr) {
  kernel<<<blocks, threads, 0, a.st>>>(a.groups, a.G, a.rp, a.src, a.orp, a.odst, a.oslot, a.Y, a.ldy, a.F, a.elr,
                                       a.attn, a.out, a.g_out, a.slope, a.gY, a.ldgy, a.C, a.gy_amax, a.gy_rows, gR,
                                       ldgr);
}

// The per-atom pair: the groups on the backward fallback list (a.G > 0) or every atom.
template <int H, int VPL>
int launch_atom_pair(const BwdArgs& a, int big) {
  const unsigned blocks = a.G > 0 ? (unsigned)a.G : (unsigned)ceil_div(a.N, kWavesPerBlock);
  gat_agg_bwd_dst_kernel<H, VPL><<<blocks, kWavesPerBlock * 64, 0, a.st>>>(
      a.N, a.groups, a.G, a.rp, a.src, a.Y, a.ldy, a.elr, a.attn, a.out, a.g_out, a.F, a.slope, a.mode, a.gpre,
      a.gY, a.ldgy, a.gY + a.C, a.ldgy, big, a.gy_amax, a.gy_rows, a.gR, a.ldgr, a.ramax);
  int rc = check_launch("gat_agg_bwd_dst_kernel");
  if (rc) return rc;
  gat_agg_bwd_src_kernel<H, VPL><<<blocks, kWavesPerBlock * 64, 0, a.st>>>(
      a.N, a.groups, a.G, a.rp, a.orp, a.odst, a.oslot, a.attn, a.gpre, a.out, a.g_out, a.F, a.mode, a.gY, a.ldgy,
      a.gY + a.C, a.ldgy, big, a.gy_amax, a.gy_rows, a.gR, a.ldgr);
  return check_launch("gat_agg_bwd_src_kernel");
}

template <int H>
int launch_bwd(bool sep, BwdArgs a) {
  const int F = a.F, mode = a.mode;
  // dR apart from gY's rows or not formed (mvml_gat_agg_bwd_res, sep): native in the source-atom
  // kernels, the LDS molecule window and the per-atom pair.  Redirected here, before anything is
  // launched: a head-mean layer always runs by source atom (mean_src = 0 as 1, at every F), and
  // the big windows are off (their groups take the per-atom pair).
  if (mode == 1 && ((option(MVML_OPT_MEAN_SRC) && F <= 1024) || sep)) return launch_mean_src<H>(a, sep);
  // flatten layer by source atom, one pass (round 5; the round-4 two-pass form — g_rst rows
  // written first, then gathered — computed the same bits and was measured slower: deleted)
  if (mode != 1 && option(MVML_OPT_FLAT_SRC)) return launch_flat_src1<H>(a);
  if (option(MVML_OPT_BWD_ATOMWISE)) a.G = 0;  // tests: the per-atom pair over every atom
  if (F % 32 == 0 && a.G > 0) {  // molecule groups: one pass over Z / g_out / dZ per group
    // 32-column chunks (two 512-thread workgroups per CU); 64-column chunks (256-B row segments,
    // half the chunks and barriers; one 1024-thread workgroup per CU) measured 1-2 % slower in
    // round 4 (profiles/r04_fwd_chunk_width.txt, second part)
    switch_const<0, 1, 2>(mode, [&](auto m) {
      constexpr int M = decltype(m)::value;
      if (!sep) launch_lds_bwd(gat_agg_bwd_lds_kernel<H, M, 32>, (unsigned)a.G, 512, a, nullptr, 0);
      else if constexpr (M != 1)  // (flatten modes: a head-mean layer left above)
        launch_lds_bwd(gat_agg_bwd_lds_kernel<H, M, 32, 512, kWinL, kECap, false, true>, (unsigned)a.G, 512, a, a.gR,
                       a.ldgr);
      return MVML_OK;
    });
    int rc = check_launch("gat_agg_bwd_lds_kernel");
    if (rc) return rc;
  } else {
    a.G = 0;  // no LDS groups: the per-atom pair covers every atom
  }
  const int big = a.G > 0 && !sep && use_big_window(H, F);
  if constexpr (H <= 4) {
    if (big) {
      switch_const<0, 1, 2>(mode, [&](auto m) {
        launch_lds_bwd(gat_agg_bwd_lds_kernel<H, decltype(m)::value, 16, kBigThreads, kPlanBigAtoms, kPlanBigEdgeCap, true>,
                       (unsigned)std::min<int64_t>(a.G, kBigBlocks), kBigThreads, a, nullptr, 0);
        return MVML_OK;
      });
      int rc = check_launch("gat_agg_bwd_lds_kernel(big)");
      if (rc) return rc;
    }
  }
  return switch_const<1, 2, 3, 4, 5, 6, 7, 8>((int)ceil_div(H * F, 256), [&](auto v) {
    return launch_atom_pair<H, decltype(v)::value>(a, big);
  });
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" size_t mvml_gat_agg_bwd_workspace_size(int64_t num_edges, int H) {
  return carve_size((size_t)num_edges * H * sizeof(float));
}

extern "C" int mvml_gat_agg_bwd(int64_t num_nodes, const int32_t* node_groups, int64_t num_groups,
                                const int32_t* in_rowptr, const int32_t* in_src,
                                const int32_t* out_rowptr, const int32_t* out_dst,
                                const int32_t* out_inslot, const float* Y, int64_t ldy,
                                const float* elr, const float* attn, const float* out,
                                const float* g_out, int H, int F, float slope, int mode, float* gY,
                                int64_t ldgy, uint32_t* gy_amax, uint32_t* gy_row_amax, void* workspace,
                                size_t workspace_bytes, void* stream) {
  clear_error();
  int rc = check_shapes(H, F, mode, ldy, Y, "gat_agg_bwd");  // Y rows hold [Z | R]
  if (rc) return rc;
  const int C = mvml_gat_proj_cols(H, F, mode == 1);
  MVML_REQUIRE(ldgy >= C + 2 * H && ldgy % 4 == 0 && ldgy < (1 << 20),
               "gat_agg_bwd: ldgy must be >= proj_cols + 2H = %d and a multiple of 4", C + 2 * H);
  return mvml_gat_agg_bwd_res(num_nodes, node_groups, num_groups, in_rowptr, in_src, out_rowptr, out_dst,
                              out_inslot, Y, ldy, elr, attn, out, g_out, H, F, slope, mode, gY, ldgy, C,
                              gY + H * F, ldgy, gy_amax, gy_row_amax, workspace, workspace_bytes, stream);
}

extern "C" int mvml_gat_agg_bwd_res(int64_t num_nodes, const int32_t* node_groups, int64_t num_groups,
                                    const int32_t* in_rowptr, const int32_t* in_src,
                                    const int32_t* out_rowptr, const int32_t* out_dst,
                                    const int32_t* out_inslot, const float* Y, int64_t ldy,
                                    const float* elr, const float* attn, const float* out,
                                    const float* g_out, int H, int F, float slope, int mode, float* gY,
                                    int64_t ldgy, int64_t elr_col, float* gR, int64_t ldgr,
                                    uint32_t* gy_amax, uint32_t* gy_row_amax, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  clear_error();
  int rc = check_shapes(H, F, mode, ldy, Y, "gat_agg_bwd", (int64_t)H * F);
  if (rc) return rc;
  const int RW = mode == 1 ? F : H * F;
  // dR inside gY's rows (the projection-row layout): the instances compiled for it, and dR
  // counts in the maxima; apart from them or not formed: the SEP forms (launch_bwd)
  const bool sep = !(gR == gY + H * F && ldgr == ldgy);
  MVML_REQUIRE(elr_col >= (sep ? H * F : H * F + RW) && ldgy >= elr_col + 2 * H && ldgy % 4 == 0 &&
                   ldgy < (1 << 20) && aligned16(gY),
               "gat_agg_bwd: gY must be 16-byte aligned, its [d el | d er] column %lld past dZ (and dR) and "
               "ldgy >= that + 2H, a multiple of 4", (long long)elr_col);
  MVML_REQUIRE(gR == nullptr || (aligned16(gR) && ldgr % 4 == 0 && ldgr >= RW && ldgr < (1 << 20)),
               "gat_agg_bwd: gR must be 16-byte aligned with a row stride ldgr >= %d that is a multiple of 4", RW);
  const int C = (int)elr_col;
  MVML_REQUIRE(attn != nullptr && elr != nullptr, "gat_agg_bwd: attn / elr from the forward are required");
  MVML_REQUIRE(mode != 0 || out != nullptr, "gat_agg_bwd: mode 0 needs the forward output");
  MVML_REQUIRE(num_groups == mvml_node_group_count(num_nodes) && (num_groups == 0 || node_groups),
               "gat_agg_bwd: node_groups must come from mvml_build_node_groups");
  if (num_nodes == 0) return MVML_OK;
  if (!workspace || workspace_bytes == 0) {
    set_error("gat_agg_bwd: workspace of mvml_gat_agg_bwd_workspace_size(E, H) bytes required");
    return MVML_ERR_WORKSPACE;
  }
  const BwdArgs a{num_nodes, node_groups, num_groups, in_rowptr, in_src, out_rowptr, out_dst, out_inslot, Y, ldy,
                  elr, attn, out, g_out, F, slope, mode, static_cast<float*>(workspace), gY, ldgy, C, gy_amax,
                  gy_row_amax, gR, ldgr, sep ? 0 : 1, as_stream(stream)};
  rc = switch_const<1, 2, 4, 8>(H, [&](auto h) { return launch_bwd<decltype(h)::value>(sep, a); });
  if (rc != kNoCase) return rc;
  set_error("gat_agg_bwd: unsupported shape");
  return MVML_ERR_INVALID;
}
