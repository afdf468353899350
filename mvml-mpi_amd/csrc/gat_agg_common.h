// What the GAT aggregation forward (gat_agg_fwd.hip) and backward (gat_agg_bwd.hip) share: the
// node-group window sizes, the streaming row accesses, the |max| bookkeeping, the fallback-list
// walk, the big windows' hub-segment tables and the entry points' shape check.
//
// Fused GAT attention + aggregation (dgl 0.9.1 GATConv.forward after fc/res_fc) and its
// atomic-free backward.  One wavefront per destination atom (two for wide layers).
//
// Projection row layout (the plain fc / res_fc GEMM, see mvml_gat_fold_weights, gat_params.hip):
//   Y[n] = [ Z (H*F) | R (RW) ]            RW = H*F (flatten modes) or F (mean mode)
// In mean mode (dgllife's last GATLayer, agg 'mean') only the head-mean of the residual is ever
// used, so the GEMM produces R_mean = X * mean_h(W_res_h)^T directly (F columns instead of H*F).
// That is GATConv's projecting res_fc.  Its other two residual kinds (dgl 0.9.1 GATConv.__init__:
// nn.Identity() when in_feats == H*F, none with residual=False) and bias=False have no residual
// columns: mvml_gat_agg_fwd_res / mvml_gat_agg_bwd_res take R (its own row stride; NULL: none),
// dR (gR; NULL: not formed) and an optional bias as arguments, and Y / gY hold [Z] / [dZ | d el |
// d er] only.  The projection-row entries are those called with R = Y + H*F, gR = gY + H*F.
// Native for a separate residual: the destination-wave forward and the LDS backward (compile-time
// SEP instances; the in-row instances are unchanged), the per-atom pair and the source-atom
// backwards (run-time gR); launch_fwd / launch_bwd redirect every other option value.
//
// Workgroup -> atom mapping is XCD-aware (xcd_block): each XCD walks one contiguous range of
// atoms, so a molecule's neighbour rows are gathered from ONE XCD's L2.
//
// Everything here sits in the unnamed namespace and is forced inline or host-side, so no kernel
// symbol comes from this header: each kernel is defined in exactly one of the two files.
#pragma once
#include "common.h"
#include "wave_ops.h"

namespace mvml {

// *out = max(*out, max_i rows[i]) (rows_amax_kernel, gat_agg_fwd.hip); nothing to do without rows / out
int launch_rows_amax(int64_t n, const uint32_t* rows, uint32_t* out, hipStream_t st);

namespace {

// streaming (non-temporal) 16-B load / store: rows read or written exactly once pass through
// without displacing the rows an XCD's waves share in L2
typedef float mvml_f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4nt(const float* p) {
  const mvml_f4v v = __builtin_nontemporal_load(reinterpret_cast<const mvml_f4v*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4nt(float* p, float4 v) {
  mvml_f4v w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<mvml_f4v*>(p));
}

// wave-uniform per-head values -> p[0..H): lane h stores a[h]
template <int H>
__device__ __forceinline__ void store_heads(float* p, const float (&a)[H], int lane) {
  if (lane < H) p[lane] = pick<H>(a, lane);
}

// |max| bookkeeping of the backward's gY stores (the split-fp16 scale of the GEMMs that read gY)
__device__ __forceinline__ float amax4(float m, float4 v) {
  return fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}
// Block |max| -> one unsigned atomicMax of the (non-negative) float bits: order-independent.
// Every thread of the block calls it (a barrier inside).
template <int NT>
__device__ __forceinline__ void block_amax_commit(float m, uint32_t* out) {
  __shared__ float red[NT / 64];
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) r = fmaxf(r, red[i]);
    atomicMax(out, __float_as_uint(r));
  }
}

// Node-group windows (mvml_build_node_groups: the group plan's kind bits and fallback lists).
constexpr int kWinL = kPlanWinAtoms;  // LDS kernel: atoms per group
constexpr int kECap = kPlanEdgeCap;   // LDS kernel: in-edges per group (attention staged in LDS)
constexpr int kEC = kPlanDegCap;      // in-edges per destination with cached offsets
// Fallback-list entry of block b in a grid of nb >= count blocks: XCD x (the blocks b % 8 == x)
// walks ONE contiguous range of the list (the lists are in group order), so the molecules in
// flight on an XCD are neighbours and their rows share its L2; -1 for idle blocks.
__device__ __forceinline__ int list_block(unsigned b, unsigned nb, int count) {
  const unsigned x = b % 8, i = b / 8;
  const unsigned q = count / 8, r = count % 8;
  const unsigned beg = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  const unsigned len = q + (x < r ? 1 : 0);
  return i < len ? (int)(beg + i) : -1;
}
constexpr int kBigThreads = 512;      // big-window kernels: 128 rows per pass (16-column chunks),
                                      // up to 4 passes; 2 waves per SIMD leave 256 registers
constexpr int kBigBlocks = 256;       // ... one workgroup per CU walking the fallback list
// Hub segments of a big window: the edges of a row past its kEC cached ones are cut into
// segments of kSegI in-edges (kSegO out-edges), each one a task for any lane group of the chunk
// sweep (a partial sum / edge dots), so a hub's 32-128 edges cost one LDS round trip per chunk
// instead of a serial walk on its own lanes.  Rows whose segments would pass the table keep the
// serial walk (correct for any graph; the tables cover config 5's 1-4 hubs per molecule).  The
// backward's out-edge partials are short of LDS: there rows of out-degree <= kSegMinO (a hub's
// partners: one or two edges past kEC, staged in s_oxe) walk theirs too.
constexpr int kSegI = 8, kSegO = 16, kSegMinO = 12;
constexpr int kSegCapI = 256, kSegCapO = 48;
constexpr int kOXCap = 640;  // backward: out-edges past kEC staged in LDS (dst row << 16 | slot)

// Block-wide exclusive prefix sum of one int per thread (NT / 64 waves); *total = the sum.
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* s_wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_wsum[w] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    const int t = s_wsum[i];
    base += i < w ? t : 0;
    tot += t;
  }
  *total = tot;
  return base + x - v;
}

// The segment table of rows d = threadIdx.x < nr (edge range [eb, eb + deg) of the window's
// CSR; rows of degree <= MIN get none): seg[t] = row << 16 | first edge << 4 | (count - 1);
// *rs = first segment | count << 12 for this thread's row (0: no segments, or segments past
// CAP: the owner walks them).  Returns the table length.  Ends with a barrier (the table is
// visible to the block).
template <int NT, int SEG, int CAP, int MIN = kEC>
__device__ __forceinline__ int hub_segments(int nr, int eb, int deg, uint32_t* s_seg, int* rs,
                                            int* s_wsum) {
  static_assert(CAP < 4096 && SEG <= 16, "segment packing");
  const int d = threadIdx.x;
  int n = (d < nr && deg > MIN) ? (deg - kEC + SEG - 1) / SEG : 0;
  int total;
  const int sb = block_excl_scan<NT>(n, s_wsum, &total);
  if (sb + n > CAP) n = 0;  // rows are in order: every later row is past the table too
  for (int j = 0; j < n; ++j) {
    const int e = eb + kEC + SEG * j;
    s_seg[sb + j] = (uint32_t)d << 16 | (uint32_t)e << 4 | (uint32_t)(min(SEG, eb + deg - e) - 1);
  }
  *rs = n ? (sb | n << 12) : 0;
  // the table length: the end of the last row that fits (a block max over the rows)
  const int end = n ? sb + n : 0;
  int m = end;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  __syncthreads();  // s_wsum reads of the scan are done
  if ((threadIdx.x & 63) == 0) s_wsum[threadIdx.x >> 6] = m;
  __syncthreads();
  int len = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) len = max(len, s_wsum[i]);
  __syncthreads();  // s_wsum reusable
  return len;
}

// The big-window kernels stage 16-column chunks (F % 16 == 0) and their LDS holds the per-edge
// attention of up to kPlanBigEdgeCap edges for H <= 4 heads.  On config 5 (8192 molecules) they
// take fwd / bwd L1 6.4 / 13.5 ms and L2 7.0 / 21.7 ms against the per-atom fallbacks' 7.0 /
// 15.9 and 10.2 / 29.7 ms.  Option MVML_OPT_BIG_WINDOW = 0 routes those groups to the
// fallbacks (tests).
inline bool use_big_window(int H, int F) {
  return option(MVML_OPT_BIG_WINDOW) != 0 && H <= 4 && F % 16 == 0;
}

// need_cols: the columns a Y row must hold (default: the projection-row layout's [Z | R])
inline int check_shapes(int H, int F, int mode, int64_t ldy, const void* Y, const char* who, int64_t need_cols = -1) {
  if (int rc = check_heads(H, F, who)) return rc;
  MVML_REQUIRE(ldy < (1 << 20), "%s: leading dimension too large", who);
  MVML_REQUIRE(mode >= 0 && mode <= 2, "%s: bad mode %d", who, mode);
  const int64_t need = need_cols >= 0 ? need_cols : (int64_t)mvml_gat_proj_cols(H, F, mode == 1);
  MVML_REQUIRE(ldy >= need && ldy % 4 == 0, "%s: leading dimension %lld < %lld or not a multiple of 4",
               who, (long long)ldy, (long long)need);
  MVML_REQUIRE(aligned16(Y), "%s: tensors must be 16-byte aligned", who);
  return MVML_OK;
}

}  // namespace
}  // namespace mvml
