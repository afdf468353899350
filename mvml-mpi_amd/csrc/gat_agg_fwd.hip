// GAT aggregation forward: the fused edge softmax + neighbour sum (row layout and residual kinds:
// gat_agg_common.h; the backward: gat_agg_bwd.hip).
//
// Forward, per destination v (rows of the in-CSR, in-edges in ascending edge id):
//   el[n,h] = <Z[n,h,:], attn_l[h,:]>, er[n,h] = <Z[n,h,:], attn_r[h,:]>   GATConv el / er, from
//             Z exactly like `(feat_src * attn_l).sum(-1)`; saved to elr[n] = [el | er]
//   s_e   = LeakyReLU(el[src_e] + er[v], slope)                apply_edges(u_add_v), leaky_relu
//   a_e   = exp(s_e - max_v s) / sum_v exp(s - max_v s)       edge_softmax (norm_by = dst)
//   rst_v = sum_e a_e * Z[src_e] + R[v] + bias                update_all(u_mul_e, sum), res, bias
//   out_v = ELU(rst_v.flatten) | mean_h(rst_v) | rst_v        dgllife GATLayer agg / activation
// el / er come from the projection GEMM (2H extra columns, elr; gat_params.hip); the edge_softmax
// runs inside the aggregation kernels (softmax_pair: one thread per destination and head, before
// the column sweep), so mvml_gat_agg_fwd is one launch per kernel kind and attn is written, never
// re-read.  (A single-pass variant that reduces el[u] from each gathered Z row with an online
// softmax was measured 2x slower: its per-edge shuffle -> exp -> rescale chain is latency-bound.)
#include "gat_agg_common.h"

namespace mvml {
namespace {

// edge_softmax of one (destination v, head h) pair inside the aggregation kernels (the same
// arithmetic and order as the round-3 standalone softmax kernel: max over the in-edges, sum of
// exp(s - max) in edge order, a_e = exp(s_e - max) / sum): writes attn[e, h] (the backward's
// input) and, when s_att is given, the group-relative copy s_att[(e - e0) H + h] the aggregation
// reads.  Logits past the register cache are recomputed in each pass (one more read of the
// L2-resident el rows; no limit on the degree).
template <int H>
__device__ __forceinline__ void softmax_pair(int64_t v, int h, const int32_t* __restrict__ rowptr,
                                             const int32_t* __restrict__ in_src,
                                             const float* __restrict__ elr, float slope,
                                             float* __restrict__ attn, float* s_att, int e0) {
  const float er = elr[v * 2 * H + H + h];
  const int eb = rowptr[v], ee = rowptr[v + 1];
  constexpr int DC = 6;
  float sc[DC];
  float m = -INFINITY, sum = 0.f;
#pragma unroll
  for (int t = 0; t < DC; ++t) {
    sc[t] = (eb + t < ee) ? leaky(elr[(int64_t)in_src[eb + t] * 2 * H + h] + er, slope) : -INFINITY;
    m = fmaxf(m, sc[t]);
  }
  for (int e = eb + DC; e < ee; ++e) m = fmaxf(m, leaky(elr[(int64_t)in_src[e] * 2 * H + h] + er, slope));
#pragma unroll
  for (int t = 0; t < DC; ++t)
    if (eb + t < ee) sum += expf(sc[t] - m);
  for (int e = eb + DC; e < ee; ++e) sum += expf(leaky(elr[(int64_t)in_src[e] * 2 * H + h] + er, slope) - m);
#pragma unroll
  for (int t = 0; t < DC; ++t)
    if (eb + t < ee) {
      const float a = expf(sc[t] - m) / sum;
      attn[(int64_t)(eb + t) * H + h] = a;
      if (s_att) s_att[(eb + t - e0) * H + h] = a;
    }
  for (int e = eb + DC; e < ee; ++e) {
    const float a = expf(leaky(elr[(int64_t)in_src[e] * 2 * H + h] + er, slope) - m) / sum;
    attn[(int64_t)e * H + h] = a;
    if (s_att) s_att[(e - e0) * H + h] = a;
  }
}

// Aggregation over NODE GROUPS.  A node group is a contiguous range of whole molecules of about
// kNodeGroupAtoms atoms (mvml_build_node_groups); edges never leave a molecule, so every in-edge
// of a group's atoms has its source inside the group, and one workgroup per group can read each
// projection row from HBM once.  The attention comes from softmax_pair.  The projection
// columns are swept CW at a time; CW/4 lanes own one destination atom (16-B column slices).
// Flatten modes walk the chunks head-major; the mean mode walks them f-chunk-major, head-minor,
// summing the heads in registers (+ bias per head, / H, + head-mean residual).
//
// Two kernels share the groups (each block decides with the same block-wide predicate):
//  * gat_agg_fwd_lds_kernel — the molecule case: a group of <= kWinL atoms, <= kECap in-edges,
//    in-degree <= kEC everywhere (organic atoms: 4 bonds + self-loop).  The group's rows are
//    streamed ONCE into an LDS double buffer through a register ring two chunks deep (chunks
//    k+1, k+2 and the next residual in flight while chunk k is aggregated, one barrier per
//    chunk); the kEC source-row LDS offsets of every destination are cached in registers, so a
//    chunk's gathers are kEC x NP independent ds_read_b128 (branch-free: a missing edge reads
//    the destination's own row and is discarded by a select) — one LDS round trip per chunk.
//  * gat_agg_fwd_gather_kernel — everything else (large molecules, hubs): no staging; the
//    gathers go straight to global memory, where the chunk-synchronous sweep keeps the group's
//    chunk rows in the XCD's L2.  Correct for any graph.
// Which kernel takes a group is decided once per batch by mvml_build_node_groups (the group
// plan: kind bits + fallback lists), so no launch scans the CSR to find its groups.
constexpr int kWin = 64;              // gather kernel: destination atoms per pass set
constexpr int kAggThreads = 512;
constexpr int kHubDeg = 16;           // gather kernel: in-degree above which the hub pass runs
constexpr int kHubCols = 1024;        // gather kernel: float4 columns of the hub pass (H*F <= 4096)
constexpr int kLdsWaves = 4;          // LDS kernel: waves per SIMD its register budget allows
constexpr int kFwdRing = 2;           // LDS kernel: chunks in flight in the register ring

// Chunk loop of the forward LDS kernel for a group of at most NPA * DPP atoms (NPA passes of
// DPP destinations).  Chunks k+1 .. k+RING are in flight in a register ring while chunk k is
// aggregated from LDS.  Loads are unconditional (rows past the group read 0 through the buffer
// resource's range check; chunks past the end use an out-of-range offset), so the loop is
// straight-line and the compiler's vmcnt waits are exact; stores of rows past the group are
// skipped (an out-of-range store is not free).
template <int H, int CW, int MODE, int NT, int NPA, int WIN = kWinL, int ECAP = kECap, bool BIG = false>
__device__ __forceinline__ float fwd_lds_chunks(float4 (*zbuf)[WIN * (CW / 4)], const float* s_att,
                                               const int32_t* __restrict__ rowptr,
                                               const int32_t* __restrict__ in_src,
                                               __amdgpu_buffer_rsrc_t rY, uint32_t rowb,
                                               __amdgpu_buffer_rsrc_t rO, int a0, int nr, int e0,
                                               int F, const float* __restrict__ bias,
                                               const uint16_t* s_srcs = nullptr,
                                               const uint32_t* s_seg = nullptr,
                                               const int* s_rs = nullptr, float4* s_part = nullptr,
                                               int nseg = 0, uint32_t* __restrict__ out_rows = nullptr) {
  constexpr int LPD = CW / 4;                        // lanes per destination atom
  constexpr int DPP = NT / LPD;                      // destinations per pass
  constexpr int RING = NPA >= 3 ? 1 : kFwdRing;      // 3-4 pass groups: registers
  const int tid = threadIdx.x;
  const int ds = tid / LPD, q = tid % LPD;
  const int HF = H * F;
  const int nfc = F / CW;     // column chunks per head
  const int nch = H * nfc;
  const int ocols = MODE == 1 ? F : HF;
  // this thread's destinations: the LDS slots of their first kEC source rows and attention
  // values; a missing edge (i >= in-degree) points at the destination's own row and at a zero
  // attention, so the edge loop is branch- and mask-free (fma(0, z, acc) == acc)
  int so[NPA][kEC], ab[NPA], ad[NPA];
  uint32_t rb[NPA], ob[NPA];  // byte offsets of this thread's rows in Y and in out
  // "no access" offsets: just past the resource's range (reads 0, drops stores) yet next to
  // the group's own rows, so the address still translates through a warm TLB entry (a wild
  // out-of-range offset costs a page walk per access)
  const uint32_t noY = (uint32_t)nr * rowb;
  float omx = 0.f;  // |max| of this thread's output stores (live rows)
  float rmx[NPA];   // ... per destination (out_rows: each row's |max|, the next GEMM's row scale)
  bool live[NPA];
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    const int d = ds + DPP * p;
    live[p] = d < nr;
    int eb = 0, deg = 0;
    if (live[p]) {
      eb = rowptr[a0 + d] - e0;
      deg = rowptr[a0 + d + 1] - e0 - eb;
    }
    ab[p] = eb * H;
    ad[p] = deg;
    rmx[p] = 0.f;
#pragma unroll
    for (int i = 0; i < kEC; ++i) {
      so[p][i] = ((i < deg) ? in_src[e0 + eb + i] - a0 : (live[p] ? d : 0)) * LPD + q;
    }
    rb[p] = (uint32_t)d * rowb;            // d >= nr: past the resource, reads 0
    ob[p] = 4u * (uint32_t)(d * ocols);
  }
  // BIG: this thread's rows' hub segments (first | count << 12); the edges of a row with none
  // past kEC are walked by the row's own lanes (hend)
  int sbn[NPA], hend[NPA];
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    sbn[p] = 0;
    if constexpr (BIG) sbn[p] = live[p] ? s_rs[ds + DPP * p] : 0;
    hend[p] = sbn[p] ? kEC : ad[p];
  }
  // chunk k -> global column of this lane
  auto col_of = [&](int k) {
    return (MODE == 1 ? (k % H) * F + (k / H) * CW : (k / nfc) * F + (k % nfc) * CW) + 4 * q;
  };
  auto load_rows = [&](int k, float4 (&dst)[NPA]) {
    const bool ok = k < nch;
    const uint32_t cb = 4u * (uint32_t)col_of(k);
#pragma unroll
    for (int j = 0; j < NPA; ++j) dst[j] = buf_ld4(rY, ok ? rb[j] + cb : noY);
  };
  // residual of chunk k (mean mode: of its f-chunk, re-read per head from L2 so that the loop
  // stays branch-free; loading it for the last head only measured slower, L2 mean 3.86 -> 4.20 ms)
  auto load_res = [&](int k, float4 (&dst)[NPA]) {
    const bool ok = k < nch;
    const uint32_t cb = 4u * (uint32_t)(HF + (MODE == 1 ? (k / H) * CW + 4 * q : col_of(k)));
#pragma unroll
    for (int j = 0; j < NPA; ++j) dst[j] = buf_ld4(rY, ok ? rb[j] + cb : noY);
  };
  auto store_rows = [&](int buf, const float4 (&src)[NPA]) {
#pragma unroll
    for (int j = 0; j < NPA; ++j) zbuf[buf][(ds + DPP * j) * LPD + q] = src[j];
  };
  // BIG emits after the barrier: chunk k's residual is loaded at the top of iteration k (no
  // second residual set in registers)
  float4 ring[RING][NPA], rres[NPA], rnx[BIG ? 1 : NPA], tot[NPA];
  {
    float4 z0[NPA];
    load_rows(0, z0);
#pragma unroll
    for (int i = 0; i < RING; ++i) load_rows(1 + i, ring[i]);
    if constexpr (!BIG) load_res(0, rres);
    store_rows(0, z0);
  }
  __syncthreads();  // chunk 0 and s_att staged
  for (int k = 0; k < nch; ++k) {
    const int h = MODE == 1 ? k % H : k / nfc;
    const int col = col_of(k);
    if constexpr (BIG) load_res(k, rres);
    else load_res(k + 1, rnx);
    const float4 b4 = ld4(bias + col);
    const float4* zl = zbuf[k & 1];
    float4 acc[NPA];
#pragma unroll
    for (int p = 0; p < NPA; ++p) acc[p] = f4(0.f);
#pragma unroll
    for (int p = 0; p < NPA; ++p)
#pragma unroll
      for (int i = 0; i < kEC; ++i)
        acc[p] = fma4(s_att[(i < ad[p] ? ab[p] + i * H : ECAP * H) + h], zl[so[p][i]], acc[p]);
    if constexpr (BIG) {
      // rows past the segment table: their in-edges past kEC on their own lanes (edge order)
#pragma unroll
      for (int p = 0; p < NPA; ++p)
        for (int i = kEC; i < hend[p]; i += 4) {
          float av[4];
          float4 zv[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool ok = i + j < ad[p];
            const int e = ab[p] / H + (ok ? i + j : i);
            av[j] = ok ? s_att[e * H + h] : 0.f;
            zv[j] = zl[(int)s_srcs[e] * LPD + q];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j < ad[p]) acc[p] = fma4(av[j], zv[j], acc[p]);
        }
      // hub segments: any lane group, kSegI independent LDS reads each; partials to s_part[k & 1]
      float4* sp = s_part + (k & 1) * (kSegCapI * LPD);
      for (int t = ds; t < nseg; t += DPP) {
        const uint32_t sg = s_seg[t];
        const int eb = (int)((sg >> 4) & 0xFFFu), c = (int)(sg & 15u) + 1;
        float4 part = f4(0.f);
#pragma unroll
        for (int j0 = 0; j0 < kSegI; j0 += 4) {  // two batches of 4 reads (registers)
          float av[4];
          float4 zv[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool ok = j0 + j < c;
            const int e = eb + (ok ? j0 + j : 0);
            av[j] = ok ? s_att[e * H + h] : 0.f;
            zv[j] = zl[(int)s_srcs[e] * LPD + q];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) part = fma4(av[j], zv[j], part);
        }
        sp[t * LPD + q] = part;
      }
    }
    auto emit = [&](int p) {
      if (MODE == 1) {
        const float4 t = add4(acc[p], b4);
        tot[p] = (h == 0) ? t : add4(tot[p], t);
        // a store whose lanes are ALL out of range still costs a real one: branch (uniform)
        if (h == H - 1) {
          const float invh = (float)H;
          const float4 o = make_float4(tot[p].x / invh + rres[p].x, tot[p].y / invh + rres[p].y,
                                       tot[p].z / invh + rres[p].z, tot[p].w / invh + rres[p].w);
          buf_st4(rO, ob[p] + 4u * (uint32_t)((k / H) * CW + 4 * q), o);
          rmx[p] = amax4(rmx[p], o);
        }
      } else {
        float4 o = add4(add4(acc[p], rres[p]), b4);
        if (MODE == 0) o = make_float4(elu(o.x), elu(o.y), elu(o.z), elu(o.w));
        buf_st4(rO, ob[p] + 4u * (uint32_t)col, o);  // rows past the group: dropped
        rmx[p] = amax4(rmx[p], o);
      }
    };
    if constexpr (!BIG) {
#pragma unroll
      for (int p = 0; p < NPA; ++p) emit(p);
    }
    // stage chunk k+1 into the other buffer (read by nobody until the barrier) and rotate
    store_rows((k + 1) & 1, ring[0]);
#pragma unroll
    for (int i = 0; i + 1 < RING; ++i)
#pragma unroll
      for (int j = 0; j < NPA; ++j) ring[i][j] = ring[i + 1][j];
    load_rows(k + 1 + RING, ring[RING - 1]);
    __syncthreads();
    if constexpr (BIG) {  // the segment partials of chunk k are complete: add them in order, emit
      const float4* sp = s_part + (k & 1) * (kSegCapI * LPD);
#pragma unroll
      for (int p = 0; p < NPA; ++p) {
        const int n = sbn[p] >> 12;
        for (int j = 0; j < n; ++j) acc[p] = add4(acc[p], sp[((sbn[p] & 0xFFF) + j) * LPD + q]);
        emit(p);
      }
    }
#pragma unroll
    for (int j = 0; j < NPA; ++j)
      if constexpr (!BIG) rres[j] = rnx[j];
  }
  // a row's |max| over its LPD lanes (consecutive lanes of one wave); one writer per row
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    float m = live[p] ? rmx[p] : 0.f;
    omx = fmaxf(omx, m);
#pragma unroll
    for (int o = LPD / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (out_rows && live[p] && q == 0) out_rows[a0 + ds + DPP * p] = __float_as_uint(m);
  }
  return omx;
}

// NT = 16 * CW threads: 64 destinations per pass; groups of <= 64 atoms (most of them: the
// target is kNodeGroupAtoms) run one pass, larger ones two (kWinL = 128 atoms).  16 waves per
// CU either way (2 x 512 threads for CW = 32, 1 x 1024 for CW = 64).
// BIG (kind bit 2): the big-window variant for the groups on the forward fallback list (config
// 5's 150-400-atom molecules with hubs): 16-column chunks so that 512 rows fit LDS, in-degree
// unbounded (the hub loop above), one workgroup per CU walking the list.
template <int H, int CW, int MODE, int NT, int WIN = kWinL, int ECAP = kECap, bool BIG = false>
__global__ void __launch_bounds__(NT, kLdsWaves)
gat_agg_fwd_lds_kernel(const int32_t* __restrict__ plan, int64_t G, const int32_t* __restrict__ rowptr,
                       const int32_t* __restrict__ in_src, const float* __restrict__ Y, int64_t ldy,
                       int F, const float* __restrict__ bias, const float* __restrict__ elr,
                       float slope, float* __restrict__ attn, float* __restrict__ out,
                       uint32_t* __restrict__ out_amax, uint32_t* __restrict__ out_rows) {
  constexpr int LPD = CW / 4;
  constexpr int DPP = NT / LPD;
  constexpr int NPM = WIN / DPP;  // passes over a full window
  static_assert(NPM * DPP == WIN && (NPM == 2 || NPM == 4), "the passes must tile the LDS rows exactly");
  __shared__ float4 zbuf[2][WIN * LPD];
  __shared__ float s_att[(ECAP + 1) * H];  // + H zeros: the attention of a missing edge
  // BIG: in-edge sources (window rows), the hub segment table, per-row segments, the
  // double-buffered segment partials and the scan's wave sums
  __shared__ uint16_t s_srcs[BIG ? ECAP : 1];
  __shared__ uint32_t s_seg[BIG ? kSegCapI : 1];
  __shared__ int s_rs[BIG ? WIN : 1];
  __shared__ float4 s_part[BIG ? 2 * kSegCapI * LPD : 1];
  __shared__ int s_wsum[BIG ? NT / 64 : 1];
  const int tid = threadIdx.x;
  const GroupPlan gp(plan, G);
  const int nlist = BIG ? gp.count[0] : (int)blockIdx.x + 1;
  float omx = 0.f;  // |max| of this thread's output stores, committed after the group loop
  for (int li = blockIdx.x; li < nlist; li += BIG ? gridDim.x : 1) {
  const int g = BIG ? gp.fwd_list[li] : li;
  if (BIG) __syncthreads();  // the previous group's LDS reads are done
  if (!(gp.kind[g] & (BIG ? 4 : 1))) continue;
  const int a0 = gp.start[g], a1 = gp.start[g + 1];
  const int nr = a1 - a0;
  const int ocols = MODE == 1 ? F : H * F;
  const int e0 = rowptr[a0];
  const int ne = rowptr[a1] - e0;
  // the group's edge_softmax, fused: one thread per (destination, head) pair into s_att (and
  // attn for the backward); fwd_lds_chunks' first barrier publishes it
  for (int pr = tid; pr < nr * H; pr += NT)
    softmax_pair<H>(a0 + pr / H, pr % H, rowptr, in_src, elr, slope, attn, s_att, e0);
  if (tid < H) s_att[ECAP * H + tid] = 0.f;
  int nseg = 0;
  if constexpr (BIG) {
    static_assert(NT >= WIN, "one row per thread for the segment scan");
    for (int i = tid; i < ne; i += NT) s_srcs[i] = (uint16_t)(in_src[e0 + i] - a0);
    const int eb = tid < nr ? rowptr[a0 + tid] - e0 : 0;
    const int deg = tid < nr ? rowptr[a0 + tid + 1] - e0 - eb : 0;
    int rs;
    nseg = hub_segments<NT, kSegI, kSegCapI>(nr, eb, deg, s_seg, &rs, s_wsum);
    if (tid < nr) s_rs[tid] = rs;
    __syncthreads();
  }
  const uint32_t rowb = (uint32_t)ldy * 4u;
  const __amdgpu_buffer_rsrc_t rY = make_rsrc(Y + (int64_t)a0 * ldy, (uint32_t)nr * rowb);
  const __amdgpu_buffer_rsrc_t rO = make_rsrc(out + (int64_t)a0 * ocols, (uint32_t)(nr * ocols) * 4u);
  if (nr <= DPP)
    omx = fmaxf(omx, fwd_lds_chunks<H, CW, MODE, NT, 1, WIN, ECAP, BIG>(zbuf, s_att, rowptr, in_src, rY, rowb, rO, a0, nr, e0, F, bias, s_srcs, s_seg, s_rs, s_part, nseg, out_rows));
  else if (NPM == 2 || nr <= 2 * DPP)
    omx = fmaxf(omx, fwd_lds_chunks<H, CW, MODE, NT, 2, WIN, ECAP, BIG>(zbuf, s_att, rowptr, in_src, rY, rowb, rO, a0, nr, e0, F, bias, s_srcs, s_seg, s_rs, s_part, nseg, out_rows));
  else if (nr <= 3 * DPP)
    omx = fmaxf(omx, fwd_lds_chunks<H, CW, MODE, NT, (NPM > 2 ? 3 : 2), WIN, ECAP, BIG>(zbuf, s_att, rowptr, in_src, rY, rowb, rO, a0, nr, e0, F, bias, s_srcs, s_seg, s_rs, s_part, nseg, out_rows));
  else
    omx = fmaxf(omx, fwd_lds_chunks<H, CW, MODE, NT, NPM, WIN, ECAP, BIG>(zbuf, s_att, rowptr, in_src, rY, rowb, rO, a0, nr, e0, F, bias, s_srcs, s_seg, s_rs, s_part, nseg, out_rows));
  }
  if (out_amax) block_amax_commit<NT>(omx, out_amax);
}

template <int H, int CW, int MODE>
__global__ void __launch_bounds__(kAggThreads, 4)  // 2 workgroups (16 waves) per CU
gat_agg_fwd_gather_kernel(const int32_t* __restrict__ plan, int64_t G, const int32_t* __restrict__ rowptr,
                   const int32_t* __restrict__ in_src, const float* __restrict__ Y, int64_t ldy,
                   int F, const float* __restrict__ bias, const float* __restrict__ elr, float slope,
                   float* __restrict__ attn, float* __restrict__ out, int skip_big,
                   uint32_t* __restrict__ out_amax, uint32_t* __restrict__ out_rows) {
  constexpr int LPD = CW / 4;                        // lanes per destination atom
  constexpr int DPP = kAggThreads / LPD;             // destinations per pass
  constexpr int NP = (kWin + DPP - 1) / DPP;         // passes over a full window
  const int tid = threadIdx.x;
  const int ds = tid / LPD, q = tid % LPD;
  const int HF = H * F;
  const GroupPlan gp(plan, G);
  const int li = list_block(blockIdx.x, gridDim.x, gp.count[0]);
  if (li < 0) return;
  const int g = gp.fwd_list[li];
  if (skip_big && (gp.kind[g] & 4)) return;  // the big-window kernel takes it
  float omx = 0.f;  // |max| of this thread's output stores (block-uniform early returns only)
  const int a0 = gp.start[g], a1 = gp.start[g + 1];
  const int nfc = F / CW;     // column chunks per head
  const int nch = H * nfc;
  const int ocols = MODE == 1 ? F : HF;
  // group-relative 32-bit byte offsets from a wave-uniform base (< 2^31: a group spans at most
  // kNodeGroupAtoms + one molecule's atoms, rows of <= 2^20 floats are checked by the host)
  const float* Yg = Y + (int64_t)a0 * ldy;
  const uint32_t rowb = (uint32_t)ldy * 4u;
  const __amdgpu_buffer_rsrc_t rY = make_rsrc(Yg, (uint32_t)(a1 - a0) * rowb);
  constexpr uint32_t kNone = 0xFFFFFFF0u;  // out of range: the load returns 0, moves no data
  // Hub destinations (in-degree > kHubDeg) leave the chunk sweep: after it, the whole block
  // aggregates one hub at a time over ALL its columns at once, so a hub costs deg / 8 memory
  // round trips instead of (column chunks) x deg / 8 on 16 lanes.  Same summation order.
  __shared__ float4 s_hub[kHubCols];
  __shared__ float s_red[kAggThreads / 64];
  const bool hubpass = HF / 4 <= kHubCols;
  // the group's edge_softmax, fused (global attn: the sweep below gathers it per edge; the
  // barrier makes this workgroup's stores visible to it)
  for (int pr = tid; pr < (a1 - a0) * H; pr += kAggThreads)
    softmax_pair<H>(a0 + pr / H, pr % H, rowptr, in_src, elr, slope, attn, nullptr, 0);
  __syncthreads();

  for (int w0 = a0; w0 < a1; w0 += kWin) {
    const int nr = min(kWin, a1 - w0);
    const int e0 = rowptr[w0];

    const float* __restrict__ attw = attn + (int64_t)e0 * H;
    const __amdgpu_buffer_rsrc_t rO = make_rsrc(out + (int64_t)w0 * ocols, (uint32_t)(nr * ocols) * 4u);
    // this thread's destinations: in-CSR ranges and the cached source-row offsets
    int eb[NP], deg[NP];
    bool hub[NP];
    uint32_t so[NP][kEC];
    int dmax = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int d = ds + DPP * p;
      eb[p] = 0;
      deg[p] = 0;
      if (d < nr) {
        eb[p] = rowptr[w0 + d] - e0;
        deg[p] = rowptr[w0 + d + 1] - e0 - eb[p];
      }
      hub[p] = hubpass && deg[p] > kHubDeg;
      if (hub[p]) deg[p] = 0;  // aggregated by the hub pass below
#pragma unroll
      for (int i = 0; i < kEC; ++i)
        so[p][i] = (i < deg[p]) ? (uint32_t)(in_src[e0 + eb[p] + i] - a0) * rowb : kNone;
      dmax = max(dmax, deg[p]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dmax = max(dmax, __shfl_xor(dmax, o, 64));  // wave-uniform
    auto att = [&](int e, int h) -> float { return attw[e * H + h]; };

    float4 tot[NP], rm[NP];
    float rmx[NP];  // per destination |max| (out_rows)
#pragma unroll
    for (int p = 0; p < NP; ++p) rmx[p] = 0.f;
    for (int k = 0; k < nch; ++k) {
      const int h = MODE == 1 ? k % H : k / nfc;
      const int fc = MODE == 1 ? k / H : k % nfc;
      const int col = h * F + fc * CW + 4 * q;
      const uint32_t colb = 4u * (uint32_t)col;
      float4 acc[NP], res[NP];
      // residual (flatten: this chunk's columns; mean: the f-chunk's head-mean columns)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int d = ds + DPP * p;
        const uint32_t rb = (d < nr) ? (uint32_t)(w0 + d - a0) * rowb : kNone;
        if (MODE != 1) res[p] = buf_ld4(rY, rb == kNone ? kNone : rb + 4u * (uint32_t)(HF + col));
        else if (h == 0) rm[p] = buf_ld4(rY, rb == kNone ? kNone : rb + 4u * (uint32_t)(HF + fc * CW + 4 * q));
      }
      // cached edges: one batch of independent loads (one memory round trip per chunk)
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p] = f4(0.f);
      {
        float4 z[NP][kEC];
        float a[NP][kEC];
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int i = 0; i < kEC; ++i) {
            z[p][i] = buf_ld4(rY, so[p][i] == kNone ? kNone : so[p][i] + colb);
            a[p][i] = (i < deg[p]) ? att(eb[p] + i, h) : 0.f;
          }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int i = 0; i < kEC; ++i)
            if (i < deg[p]) acc[p] = fma4(a[p][i], z[p][i], acc[p]);
      }
      if (dmax > kEC) {  // hubs: batches of 8 independent gathers (same summation order)
#pragma unroll
        for (int p = 0; p < NP; ++p)
          for (int i = kEC; i < deg[p]; i += 8) {
            uint32_t ob[8];
            float av[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const bool ok = i + j < deg[p];
              const int e = eb[p] + (ok ? i + j : i);
              ob[j] = ok ? (uint32_t)(in_src[e0 + e] - a0) * rowb + colb : kNone;
              av[j] = ok ? att(e, h) : 0.f;
            }
            float4 zv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) zv[j] = buf_ld4(rY, ob[j]);
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (i + j < deg[p]) acc[p] = fma4(av[j], zv[j], acc[p]);
          }
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int d = ds + DPP * p;
        if (d < nr && !hub[p]) {
          if (MODE == 1) {
            const float4 t = add4(acc[p], ld4(bias + col));
            tot[p] = (h == 0) ? t : add4(tot[p], t);
            if (h == H - 1) {
              const float invh = (float)H;
              const float4 o = make_float4(tot[p].x / invh + rm[p].x, tot[p].y / invh + rm[p].y,
                                           tot[p].z / invh + rm[p].z, tot[p].w / invh + rm[p].w);
              buf_st4(rO, 4u * (uint32_t)(d * F + fc * CW + 4 * q), o);
              rmx[p] = amax4(rmx[p], o);
            }
          } else {
            float4 o = add4(add4(acc[p], res[p]), ld4(bias + col));
            if (MODE == 0) o = make_float4(elu(o.x), elu(o.y), elu(o.z), elu(o.w));
            buf_st4(rO, 4u * (uint32_t)(d * HF + col), o);
            rmx[p] = amax4(rmx[p], o);
          }
        }
      }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {  // rows of the sweep: |max| over their LPD lanes, one writer
      const int d = ds + DPP * p;
      float m = rmx[p];
      omx = fmaxf(omx, m);
#pragma unroll
      for (int o = LPD / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      if (out_rows && d < nr && !hub[p] && q == 0) out_rows[w0 + d] = __float_as_uint(m);
    }
    if (!hubpass) continue;
    for (int d = 0; d < nr; ++d) {  // block-uniform walk over the window's hubs
      const int hb = rowptr[w0 + d] - e0, hdeg = rowptr[w0 + d + 1] - e0 - hb;
      if (hdeg <= kHubDeg) continue;
      const uint32_t vb = (uint32_t)(w0 + d - a0) * rowb;
      float hmx = 0.f;  // this thread's part of the hub row's |max|
      for (int c4 = tid; c4 < HF / 4; c4 += kAggThreads) {
        const int col = 4 * c4, h = col / F;
        const uint32_t colb = 4u * (uint32_t)col;
        float4 acc = f4(0.f);
        for (int i = 0; i < hdeg; i += 8) {
          uint32_t ob[8];
          float av[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const bool ok = i + j < hdeg;
            const int e = hb + (ok ? i + j : i);
            ob[j] = ok ? (uint32_t)(in_src[e0 + e] - a0) * rowb + colb : kNone;
            av[j] = ok ? attw[e * H + h] : 0.f;
          }
          float4 zv[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) zv[j] = buf_ld4(rY, ob[j]);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (i + j < hdeg) acc = fma4(av[j], zv[j], acc);
        }
        if (MODE == 1) {
          s_hub[c4] = add4(acc, ld4(bias + col));
        } else {
          const float4 res = buf_ld4(rY, vb + 4u * (uint32_t)(HF + col));
          float4 o = add4(add4(acc, res), ld4(bias + col));
          if (MODE == 0) o = make_float4(elu(o.x), elu(o.y), elu(o.z), elu(o.w));
          buf_st4(rO, 4u * (uint32_t)(d * HF + col), o);
          hmx = amax4(hmx, o);
        }
      }
      if (MODE == 1) {  // head mean, heads summed in order as in the chunk sweep
        __syncthreads();
        for (int f4 = tid; f4 < F / 4; f4 += kAggThreads) {
          float4 tot = s_hub[f4];
          for (int hh = 1; hh < H; ++hh) tot = add4(tot, s_hub[hh * (F / 4) + f4]);
          const float4 rmv = buf_ld4(rY, vb + 4u * (uint32_t)(HF + 4 * f4));
          const float invh = (float)H;
          const float4 o = make_float4(tot.x / invh + rmv.x, tot.y / invh + rmv.y,
                                       tot.z / invh + rmv.z, tot.w / invh + rmv.w);
          buf_st4(rO, 4u * (uint32_t)(d * F + 4 * f4), o);
          hmx = amax4(hmx, o);
        }
        __syncthreads();
      }
      omx = fmaxf(omx, hmx);
      if (out_rows) {  // the hub row's |max| over the block (block-uniform branch)
        hmx = wave_max(hmx);
        if ((tid & 63) == 0) s_red[tid >> 6] = hmx;
        __syncthreads();
        if (tid == 0) {
          float m = s_red[0];
#pragma unroll
          for (int w = 1; w < kAggThreads / 64; ++w) m = fmaxf(m, s_red[w]);
          out_rows[w0 + d] = __float_as_uint(m);
        }
        __syncthreads();
      }
    }
  }
  if (out_amax) block_amax_commit<kAggThreads>(omx, out_amax);
}

// ---- Forward by destination wave (MVML_OPT_DST_FWD) -------------------------------------------
// One wave per destination atom v.  xcd_block hands each XCD one contiguous atom range, so the
// projection rows a destination gathers were just read by its neighbours' waves and come from
// the XCD's L2 (tree / ring edges), or from the Infinity Cache (a hub's partners); each row
// crosses HBM about once.  SM (fused softmax): the wave forms v's edge softmax with its lanes on
// the in-edges (softmax_pair's arithmetic and order: max, then the sum of exp in edge order,
// a = exp / sum) and writes attn; !SM: gat_softmax_dst_kernel wrote attn before, and the wave
// reads it (one dependent load less per atom).  Then it gathers the WHOLE Z[src] row of each
// in-edge into registers, U rows in flight, sums them in edge order starting from 0 (bitwise the
// LDS / gather kernels' sums), adds residual and bias, applies ELU or the head mean and writes
// out[v] once.  No LDS, no barriers, no size classes: one code path for every molecule size.
// Column slots: flatten modes: lane l owns float4 columns c = l + 64 j (j < NJ, 4c < H F);
// mean mode (H >= 2): the two half-waves own heads [0, H/2) and [H/2, H), lane l the f-float4
// columns q = (l & 31) + 32 k (k < NJ, 4q < F) of its half's heads (6 slots per lane at
// H = 4, F = 384, no idle lane), and the halves meet by a cross-half shuffle for the head sum,
// added in head order (bitwise the LDS kernel's head mean).  H = 1 mean: q = l + 64 k.
// LR (late residual): the residual row is loaded after the gather instead of before the softmax
// (12 fewer VGPRs live across the gather loop in mean mode: five waves per SIMD instead of four)
// (measured: the head-mean form held to six waves per SIMD spills 17 VGPRs with the fused softmax
// and ran 6.1 -> 7.6-8.1 ms on config 5; even without it)
// SEP (mvml_gat_agg_fwd_res): the residual rows come from R (row stride ldr; NULL: no residual)
// instead of Y's columns past H F, and bias may be NULL.  !SEP is the in-row layout with a
// bias, compiled exactly as before (R / ldr unused).
template <int H, int MODE, int NJ, int U, bool SM, bool LR = false, bool SEP = false>
__global__ void __launch_bounds__(256, LR ? (MODE == 1 ? 5 : 8) : 1)
gat_agg_fwd_dst_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ in_src,
                       const float* __restrict__ Y, int64_t ldy, int F, const float* __restrict__ bias,
                       const float* __restrict__ elr, float slope, float* __restrict__ attn,
                       float* __restrict__ out, uint32_t* __restrict__ out_amax,
                       uint32_t* __restrict__ out_rows, const float* __restrict__ R = nullptr,
                       int64_t ldr = 0) {
  constexpr bool PAIR = MODE == 1 && H >= 2;
  constexpr int NH = PAIR ? H / 2 : 1;  // heads per lane (mean mode); 1 register set (flatten)
  const int lane = threadIdx.x & 63;
  const int64_t v = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float omx = 0.f;
  // (a non-persistent grid: the dispatcher hands out blocks in atom order, which keeps an XCD's
  // waves on one compact window of neighbouring atoms; a persistent walk let them drift apart
  // and ran 1.3-1.7x slower on config 5)
  if (v < N) {  // (no early return: block_amax_commit below has a barrier)
    const int HF = H * F;
    const int hp = PAIR ? lane >> 5 : 0;       // mean: this lane's half (heads hp H/2 ..)
    const int ql = PAIR ? (lane & 31) : lane;  // mean: f-float4 base of this lane
    const float* yv = Y + v * ldy;
    // this atom's residual row (SEP: NULL without a residual) and the bias (SEP: may be NULL)
    const float* rv = SEP ? (R ? R + v * ldr : nullptr) : yv + HF;
    auto ldres = [&](int c) -> float4 {
      if constexpr (SEP) return rv ? ld4nt(rv + c) : f4(0.f);
      else return ld4nt(rv + c);
    };
    auto ldbias = [&](int c) -> float4 {
      if constexpr (SEP) return bias ? ld4(bias + c) : f4(0.f);
      else return ld4(bias + c);
    };
    bool ok[NJ];
    int hc[NJ];   // flatten: the head of each column slot
    int cz[NJ];   // float offset of slot j in a projection row (mean: of head hp * NH)
    float4 res[NJ], acc[NH][NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if constexpr (MODE == 1) {
        const int q = ql + (PAIR ? 32 : 64) * j;
        ok[j] = 4 * q < F;
        hc[j] = 0;
        cz[j] = hp * NH * F + 4 * q;
        // the residual first (its HBM latency overlaps the softmax); the lower half stores out
        if constexpr (!LR) res[j] = (ok[j] && hp == 0) ? ldres(4 * q) : f4(0.f);
      } else {
        const int c = lane + 64 * j;
        ok[j] = 4 * c < HF;
        hc[j] = ok[j] ? 4 * c / F : 0;
        cz[j] = 4 * c;
        if constexpr (!LR) res[j] = ok[j] ? ldres(4 * c) : f4(0.f);
      }
#pragma unroll
      for (int h = 0; h < NH; ++h) acc[h][j] = f4(0.f);
    }
    const int eb = rowptr[v], deg = rowptr[v + 1] - eb;
    float er[H], m[H], sum[H], s0[H];
    int src0 = 0;
    // logits of the in-edges [eb + base, ...) on the lanes (edge order); -inf past the row
    auto logits = [&](int base, int& src, float (&s)[H]) {
      const bool in = base + lane < deg;
      src = in ? in_src[eb + base + lane] : 0;
#pragma unroll
      for (int h = 0; h < H; ++h)
        s[h] = in ? leaky(elr[(int64_t)src * 2 * H + h] + er[h], slope) : -INFINITY;
    };
    if constexpr (SM) {
#pragma unroll
      for (int h = 0; h < H; ++h) er[h] = elr[v * 2 * H + H + h];
      logits(0, src0, s0);
#pragma unroll
      for (int h = 0; h < H; ++h) m[h] = s0[h];
      for (int base = 64; base < deg; base += 64) {  // in-degree > 64 (hubs): more chunks
        int s_;
        float s[H];
        logits(base, s_, s);
#pragma unroll
        for (int h = 0; h < H; ++h) m[h] = fmaxf(m[h], s[h]);
      }
      HeadReduce<H>::template all<true>(m, lane);
      // sum of exp in edge order (softmax_pair's order), lane by lane
#pragma unroll
      for (int h = 0; h < H; ++h) sum[h] = 0.f;
      for (int base = 0; base < deg; base += 64) {
        int s_ = src0;
        float s[H];
        if (base == 0) {
#pragma unroll
          for (int h = 0; h < H; ++h) s[h] = s0[h];
        } else {
          logits(base, s_, s);
        }
        float p[H];
#pragma unroll
        for (int h = 0; h < H; ++h) p[h] = base + lane < deg ? expf(s[h] - m[h]) : 0.f;
        const int cnt = min(64, deg - base);
        for (int i = 0; i < cnt; ++i)
#pragma unroll
          for (int h = 0; h < H; ++h) sum[h] += rl(p[h], i);
      }
    } else {
      src0 = lane < deg ? in_src[eb + lane] : 0;
    }
    // (the attention of) the in-edges and the gather, 64 edges per chunk
    for (int base = 0; base < deg; base += 64) {
      const int cnt = min(64, deg - base);
      int src_l = src0;
      float a_l[H];
      if constexpr (SM) {
        float s[H];
        if (base == 0) {
#pragma unroll
          for (int h = 0; h < H; ++h) s[h] = s0[h];
        } else {
          logits(base, src_l, s);
        }
#pragma unroll
        for (int h = 0; h < H; ++h) a_l[h] = lane < cnt ? expf(s[h] - m[h]) / sum[h] : 0.f;
        if (lane < cnt) {
          float* ap = attn + (int64_t)(eb + base + lane) * H;
          if constexpr (H == 4) {
            st4(ap, make_float4(a_l[0], a_l[1], a_l[2], a_l[3]));
          } else {
#pragma unroll
            for (int h = 0; h < H; ++h) ap[h] = a_l[h];
          }
        }
      } else {
        if (base > 0) src_l = lane < cnt ? in_src[eb + base + lane] : 0;
        const float* ap = attn + (int64_t)(eb + base + lane) * H;
        if constexpr (H == 4) {
          const float4 a4 = lane < cnt ? ld4(ap) : f4(0.f);
          a_l[0] = a4.x; a_l[1] = a4.y; a_l[2] = a4.z; a_l[3] = a4.w;
        } else {
#pragma unroll
          for (int h = 0; h < H; ++h) a_l[h] = lane < cnt ? ap[h] : 0.f;
        }
      }
      for (int j0 = 0; j0 < cnt; j0 += U) {
        float4 z[U][NH][NJ];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = min(j0 + u, cnt - 1);  // past the chunk: a duplicate row, not summed
          const float* zr = Y + (int64_t)rl(src_l, e) * ldy;
#pragma unroll
          for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int j = 0; j < NJ; ++j) z[u][h][j] = ok[j] ? ld4(zr + cz[j] + h * F) : f4(0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (j0 + u < cnt) {  // (uniform)
            float a[H];
#pragma unroll
            for (int h = 0; h < H; ++h) a[h] = rl(a_l[h], j0 + u);
#pragma unroll
            for (int h = 0; h < NH; ++h) {
              // mean: this half's head hp NH + h (a select between the halves' heads)
              float ah = a[h];
              if constexpr (PAIR) ah = hp ? a[NH + h] : a[h];
#pragma unroll
              for (int j = 0; j < NJ; ++j)
                acc[h][j] = fma4(MODE == 1 ? ah : pick<H>(a, hc[j]), z[u][h][j], acc[h][j]);
            }
          }
        }
      }
    }
    float rmx = 0.f;
    if constexpr (LR) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if constexpr (MODE == 1) {
          const int q = ql + (PAIR ? 32 : 64) * j;
          res[j] = (ok[j] && hp == 0) ? ldres(4 * q) : f4(0.f);
        } else {
          res[j] = ok[j] ? ldres(4 * (lane + 64 * j)) : f4(0.f);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float4 o;
      if constexpr (MODE == 1) {  // head mean: heads summed in order (+ bias per head), / H, + R
        const int q = ql + (PAIR ? 32 : 64) * j;
        const int qc = ok[j] ? 4 * q : 0;
        float4 t[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) t[h] = add4(acc[h][j], ldbias((hp * NH + h) * F + qc));
        float4 tot = t[0];
#pragma unroll
        for (int h = 1; h < NH; ++h) tot = add4(tot, t[h]);
        if constexpr (PAIR) {  // + the upper half's heads, in order
#pragma unroll
          for (int h = 0; h < NH; ++h)
            tot = add4(tot, make_float4(__shfl_xor(t[h].x, 32, 64), __shfl_xor(t[h].y, 32, 64),
                                        __shfl_xor(t[h].z, 32, 64), __shfl_xor(t[h].w, 32, 64)));
        }
        if (!ok[j] || hp != 0) continue;
        const float invh = (float)H;
        o = make_float4(tot.x / invh + res[j].x, tot.y / invh + res[j].y, tot.z / invh + res[j].z,
                        tot.w / invh + res[j].w);
        st4nt(out + v * F + 4 * q, o);
      } else {
        if (!ok[j]) continue;
        o = add4(add4(acc[0][j], res[j]), ldbias(cz[j]));
        if (MODE == 0) o = make_float4(elu(o.x), elu(o.y), elu(o.z), elu(o.w));
        st4nt(out + v * HF + cz[j], o);
      }
      rmx = amax4(rmx, o);
    }
    const float wm = wave_max(rmx);
    omx = fmaxf(omx, wm);
    if (out_rows && lane == 0) out_rows[v] = __float_as_uint(wm);
  }
  if (out_amax) block_amax_commit<256>(omx, out_amax);
}

// *out = max(*out, max_i rows[i]) (bits of non-negative floats): the operand max of a product
// from the per-row maxima its producer already wrote, instead of one atomicMax per 4-atom block
// of a wave-per-atom kernel (a single word takes ~90 atomics per us: 440 k of them were most of
// the forward's 5 ms on config 5).  A few hundred blocks, one atomic each.
__global__ void __launch_bounds__(256)
rows_amax_kernel(int64_t n, const uint32_t* __restrict__ rows, uint32_t* __restrict__ out) {
  uint32_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    m = max(m, rows[i]);
  block_amax_commit<256>(__uint_as_float(m), out);
}

// H = 4: one thread per destination with the four heads as one float4 (el / er rows are 16 B),
// softmax_pair's per-head arithmetic and edge order, so attn is bitwise the same; the first DC
// logits stay in registers, later ones are recomputed (L2-resident el rows).
__global__ void __launch_bounds__(256)
gat_softmax_dst4_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ in_src,
                        const float* __restrict__ elr, float slope, float* __restrict__ attn) {
  const int64_t v = xcd_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (v >= N) return;
  const float4 er = ld4(elr + v * 8 + 4);
  const int eb = rowptr[v], ee = rowptr[v + 1];
  auto logit = [&](int e) {
    const float4 el = ld4(elr + (int64_t)in_src[e] * 8);
    return make_float4(leaky(el.x + er.x, slope), leaky(el.y + er.y, slope), leaky(el.z + er.z, slope),
                       leaky(el.w + er.w, slope));
  };
  constexpr int DC = 6;
  float4 sc[DC];
  float4 m = f4(-INFINITY), sum = f4(0.f);
#pragma unroll
  for (int t = 0; t < DC; ++t) {
    sc[t] = (eb + t < ee) ? logit(eb + t) : f4(-INFINITY);
    m = make_float4(fmaxf(m.x, sc[t].x), fmaxf(m.y, sc[t].y), fmaxf(m.z, sc[t].z), fmaxf(m.w, sc[t].w));
  }
  for (int e = eb + DC; e < ee; ++e) {
    const float4 c = logit(e);
    m = make_float4(fmaxf(m.x, c.x), fmaxf(m.y, c.y), fmaxf(m.z, c.z), fmaxf(m.w, c.w));
  }
  auto ex = [&](float4 c) {
    return make_float4(expf(c.x - m.x), expf(c.y - m.y), expf(c.z - m.z), expf(c.w - m.w));
  };
#pragma unroll
  for (int t = 0; t < DC; ++t)
    if (eb + t < ee) sum = add4(sum, ex(sc[t]));
  for (int e = eb + DC; e < ee; ++e) sum = add4(sum, ex(logit(e)));
  auto store = [&](int e, float4 c) {
    const float4 p = ex(c);
    st4(attn + (int64_t)e * 4, make_float4(p.x / sum.x, p.y / sum.y, p.z / sum.z, p.w / sum.w));
  };
#pragma unroll
  for (int t = 0; t < DC; ++t)
    if (eb + t < ee) store(eb + t, sc[t]);
  for (int e = eb + DC; e < ee; ++e) store(e, logit(e));
}

// The edge softmax alone, one thread per (destination, head) (softmax_pair: bitwise the fused
// kernels' attn), for gat_agg_fwd_dst_kernel<..., SM = false>.
template <int H>
__global__ void __launch_bounds__(256)
gat_softmax_dst_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ in_src,
                       const float* __restrict__ elr, float slope, float* __restrict__ attn) {
  const int64_t i = xcd_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (i >= N * H) return;
  softmax_pair<H>(i / H, (int)(i % H), rowptr, in_src, elr, slope, attn, nullptr, 0);
}

// ---------------------------------------------------------------------------------- dispatch
// One forward: what every kernel family reads.  R / ldr: the residual rows of the SEP instances
// (mvml_gat_agg_fwd_res; NULL, 0 in the projection-row layout, whose instances ignore them).
struct FwdArgs {
  int64_t N;
  const int32_t* groups;
  int64_t G;
  const int32_t *rp, *src;
  const float* Y;
  int64_t ldy;
  int F;
  const float *bias, *elr;
  float slope;
  int mode;
  float *out, *attn;
  uint32_t *out_amax, *out_rows;
  const float* R;
  int64_t ldr;
  hipStream_t st;
};

// The destination-wave instance of a shape, <H, M, NJ, U, SM, LR, SEP>, is a function of its
// column slots per lane NJ.  U, projection rows in flight per wave: fewer rows in flight, more
// waves, is faster from three slots on (one row: fewest registers, most waves).
constexpr int dst_rows_in_flight(int M, int NJ) {
  return NJ == 1 ? 4 : NJ == 2 ? (M == 1 ? 2 : 4) : NJ == 3 ? 1 : NJ == 4 ? 2 : (M == 1 ? 1 : 2);
}
// LR, the residual loaded after the gather: H = 4 at three slots (the GAT widths), in-row layout.
// Head mean: 90 VGPRs, five waves per SIMD (residual first: 104, four) — config 5 layer 2
// 6.35 -> 6.08 ms, config 3 3.66 -> 3.60 (profiles/r05_agg_late_residual_config*.txt).
// Flatten: 60 VGPRs, eight waves per SIMD instead of six; with the fused softmax (large
// molecules) config-5 layer 1 4.90 -> 4.41 ms, the split-softmax form (small molecules) measured
// even and keeps the residual first (profiles/r05_agg_late_residual_flatten_config*.txt).
constexpr bool dst_late_residual(int H, int M, int NJ, bool SEP, bool SM) {
  return !SEP && H == 4 && NJ == 3 && (M == 1 || SM);
}

template <int H, int M, int NJ, bool SEP>
int launch_dst_fwd(bool sm, const FwdArgs& a) {
  constexpr int U = dst_rows_in_flight(M, NJ);
  const auto kernel = sm ? gat_agg_fwd_dst_kernel<H, M, NJ, U, true, dst_late_residual(H, M, NJ, SEP, true), SEP>
                         : gat_agg_fwd_dst_kernel<H, M, NJ, U, false, dst_late_residual(H, M, NJ, SEP, false), SEP>;
  // with per-row maxima requested, max |out| comes from them afterwards (no per-block atomics)
  kernel<<<(unsigned)ceil_div(a.N, 4), 256, 0, a.st>>>(a.N, a.rp, a.src, a.Y, a.ldy, a.F, a.bias, a.elr, a.slope,
                                                       a.attn, a.out, a.out_rows ? nullptr : a.out_amax,
                                                       a.out_rows, a.R, a.ldr);
  return check_launch("gat_agg_fwd_dst_kernel");
}

// One wave per destination atom, every atom.  Mean mode: half-waves over the heads, lanes over
// F / 4; flatten modes: lanes over H F / 4.  Shapes past four slots take the 8-slot instance.
template <int H, bool SEP>
int launch_dst_fwd_shape(bool sm, const FwdArgs& a) {
  const int nj = a.mode == 1 ? (int)ceil_div(a.F / 4, H >= 2 ? 32 : 64) : (int)ceil_div(H * a.F / 4, 64);
  const int rc = switch_const<0, 1, 2>(a.mode, [&](auto m) {
    return switch_const<1, 2, 3, 4, 8>(nj <= 4 ? nj : 8, [&](auto s) {
      constexpr int M = decltype(m)::value, NJ = decltype(s)::value;
      // head-mean rows past 4 slots (F > 512 at H = 2, 1024 at H = 1): a separate residual and
      // H <= 2 only (in the projection-row layout launch_fwd's dst_fits keeps them away)
      if constexpr (M == 1 && NJ == 8 && !(SEP && H <= 2)) return kNoCase;
      else return launch_dst_fwd<H, M, NJ, SEP>(sm, a);
    });
  });
  if (rc) return rc;
  return launch_rows_amax(a.N, a.out_rows, a.out_amax, a.st);
}

// The node-group kernels at chunk width CW: the LDS window, the gather kernel for the groups on
// the fallback list and, with big, the big window for those among them that fit it.
template <int H, int CW, int M>
void launch_group_fwd(bool big, const FwdArgs& a) {
  gat_agg_fwd_lds_kernel<H, CW, M, CW * 16><<<(unsigned)a.G, CW * 16, 0, a.st>>>(
      a.groups, a.G, a.rp, a.src, a.Y, a.ldy, a.F, a.bias, a.elr, a.slope, a.attn, a.out, a.out_amax, a.out_rows);
  gat_agg_fwd_gather_kernel<H, CW, M><<<(unsigned)a.G, kAggThreads, 0, a.st>>>(
      a.groups, a.G, a.rp, a.src, a.Y, a.ldy, a.F, a.bias, a.elr, a.slope, a.attn, a.out, big, a.out_amax,
      a.out_rows);
  if constexpr (H <= 4)
    if (big)
      gat_agg_fwd_lds_kernel<H, 16, M, kBigThreads, kPlanBigAtoms, kPlanBigEdgeCap, true>
          <<<(unsigned)std::min<int64_t>(a.G, kBigBlocks), kBigThreads, 0, a.st>>>(
              a.groups, a.G, a.rp, a.src, a.Y, a.ldy, a.F, a.bias, a.elr, a.slope, a.attn, a.out, a.out_amax,
              a.out_rows);
}

template <int H>
int launch_fwd(bool sep, const FwdArgs& a) {
  const int F = a.F;
  // The edge softmax as a launch of its own before the destination waves (dst_fwd = 2).
  auto softmax_first = [&](bool dst4) {
    if (dst4) {
      gat_softmax_dst4_kernel<<<(unsigned)ceil_div(a.N, 256), 256, 0, a.st>>>(a.N, a.rp, a.src, a.elr, a.slope, a.attn);
      return check_launch("gat_softmax_dst4_kernel");
    }
    gat_softmax_dst_kernel<H><<<(unsigned)ceil_div(a.N * H, 256), 256, 0, a.st>>>(a.N, a.rp, a.src, a.elr, a.slope, a.attn);
    return check_launch("gat_softmax_dst_kernel");
  };
  // A residual apart from Y's rows, no residual or no bias (mvml_gat_agg_fwd_res): the
  // destination-wave kernel's SEP instances are the one native path, at every shape (head-mean
  // rows past 4 slots, H <= 2 only, take an 8-slot instance); every option value is redirected
  // to them here, before anything is launched (dst_fwd 0 runs as 1: the softmax in the wave).
  if (sep) {
    const bool sm = option(MVML_OPT_DST_FWD) != 2;
    if (!sm)
      if (int rc = softmax_first(false)) return rc;
    return launch_dst_fwd_shape<H, true>(sm, a);
  }
  // The destination-wave kernel holds at most 4 float4 column slots per lane in mean mode (half-
  // waves over the heads for H >= 2: F <= 512; H = 1: F <= 1024) and 8 in the flatten modes
  // (H F <= 2048).  Wider head-mean shapes take the window / gather kernels below, whatever the
  // option says: decided here, before anything is launched.
  const bool dst_fits = H * F <= 2048 && (a.mode != 1 || ceil_div(F / 4, H >= 2 ? 32 : 64) <= 4);
  if (option(MVML_OPT_DST_FWD) && dst_fits) {
    const bool sm = option(MVML_OPT_DST_FWD) == 1;  // 2: the softmax as its own launch first
    if (!sm)
      if (int rc = softmax_first(H == 4)) return rc;
    return launch_dst_fwd_shape<H, false>(sm, a);
  }
  if (a.G == 0) return MVML_OK;
  const bool big = use_big_window(H, F);
  // The edge_softmax runs inside each kernel for its own groups (no separate softmax launch).
  // Widest column chunk of the LDS kernel: 32 (two 512-thread workgroups per CU, so one group's
  // softmax and first loads overlap the other's chunk sweep) measured 3-5 % faster than 64 (one
  // 1024-thread workgroup per CU) on configs 2 and 3 (profiles/r04_fwd_chunk_width.txt).
  const int cw = F % 32 == 0 ? 32 : F % 16 == 0 ? 16 : F % 8 == 0 ? 8 : 4;
  switch_const<4, 8, 16, 32>(cw, [&](auto c) {
    return switch_const<0, 1, 2>(a.mode, [&](auto m) {
      launch_group_fwd<H, decltype(c)::value, decltype(m)::value>(big, a);
      return MVML_OK;
    });
  });
  return check_launch("gat_agg_fwd_kernel");
}

}  // namespace

int launch_rows_amax(int64_t n, const uint32_t* rows, uint32_t* out, hipStream_t st) {
  if (!rows || !out || n <= 0) return MVML_OK;
  rows_amax_kernel<<<(unsigned)std::min<int64_t>(ceil_div(n, 256 * 16), 512), 256, 0, st>>>(n, rows, out);
  return check_launch("rows_amax_kernel");
}

}  // namespace mvml

using namespace mvml;

extern "C" int mvml_gat_agg_fwd(int64_t num_nodes, const int32_t* node_groups, int64_t num_groups,
                                const int32_t* in_rowptr, const int32_t* in_src, const float* Y,
                                int64_t ldy, int H, int F, const float* elr, const float* bias,
                                float slope, int mode, float* out, float* attn, uint32_t* out_amax,
                                uint32_t* out_row_amax, void* stream) {
  clear_error();
  int rc = check_shapes(H, F, mode, ldy, Y, "gat_agg_fwd");  // Y rows hold [Z | R]
  if (rc) return rc;
  return mvml_gat_agg_fwd_res(num_nodes, node_groups, num_groups, in_rowptr, in_src, Y, ldy, H, F, elr,
                              Y + H * F, ldy, bias, slope, mode, out, attn, out_amax, out_row_amax, stream);
}

extern "C" int mvml_gat_agg_fwd_res(int64_t num_nodes, const int32_t* node_groups, int64_t num_groups,
                                    const int32_t* in_rowptr, const int32_t* in_src, const float* Y,
                                    int64_t ldy, int H, int F, const float* elr, const float* R,
                                    int64_t ldr, const float* bias, float slope, int mode, float* out,
                                    float* attn, uint32_t* out_amax, uint32_t* out_row_amax,
                                    void* stream) {
  clear_error();
  int rc = check_shapes(H, F, mode, ldy, Y, "gat_agg_fwd", (int64_t)H * F);
  if (rc) return rc;
  const int RW = mode == 1 ? F : H * F;
  MVML_REQUIRE(aligned16(out) && aligned16(bias),
               "gat_agg_fwd: out / bias must be 16-byte aligned");
  MVML_REQUIRE(R == nullptr || (aligned16(R) && ldr % 4 == 0 && ldr >= RW && ldr < (1 << 20)),
               "gat_agg_fwd: R must be 16-byte aligned with a row stride ldr >= %d that is a multiple of 4", RW);
  // the projection-row layout with a bias runs the instances compiled for it; a residual apart
  // from Y, no residual or no bias the SEP ones (launch_fwd)
  const bool sep = !(R == Y + H * F && ldr == ldy && bias != nullptr);
  MVML_REQUIRE(attn != nullptr && elr != nullptr, "gat_agg_fwd: elr input and attn output are required");
  MVML_REQUIRE(num_groups == mvml_node_group_count(num_nodes) && (num_groups == 0 || node_groups),
               "gat_agg_fwd: node_groups must come from mvml_build_node_groups (%lld groups expected)",
               (long long)mvml_node_group_count(num_nodes));
  if (num_nodes == 0) return MVML_OK;
  const FwdArgs a{num_nodes, node_groups, num_groups, in_rowptr, in_src, Y, ldy, F, bias, elr, slope, mode, out,
                  attn, out_amax, out_row_amax, sep ? R : nullptr, sep ? ldr : 0, as_stream(stream)};
  rc = switch_const<1, 2, 4, 8>(H, [&](auto h) { return launch_fwd<decltype(h)::value>(sep, a); });
  if (rc != kNoCase) return rc;
  set_error("gat_agg_fwd: unsupported shape");
  return MVML_ERR_INVALID;
}
