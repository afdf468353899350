// GraphConv's aggregation (dgl 0.9.1 GraphConv.forward: update_all(copy_u, sum) between its two
// degree normalisations) and the degree factors themselves.
//
//   out[v] = act( row_scale[v] * sum_s nbr_scale[nbr[s]] * X[nbr[s]] + bias ),  s over v's CSR row
//
// One entry serves both directions: the forward walks the in-CSR (nbr_scale = the sources'
// factors, row_scale = the destinations'), the input gradient of the sum walks the out-CSR with
// the two scales swapped and no bias or act.  Both are gathers, so nothing is accumulated with
// atomics and every result is bitwise repeatable.
//
// The kernel has gat_agg_fwd_dst_kernel's form (gat_agg_fwd.hip) without the softmax: one wave per
// row v (xcd_block: an XCD walks one contiguous row range, so the neighbour rows a wave gathers
// were just read by its neighbours' waves and come from that XCD's L2), lanes on the float4
// columns c = lane + 64 j with the last slot masked, the neighbour ids loaded 64 per chunk onto
// the lanes and broadcast by readlane, whole neighbour rows gathered into registers (U in flight)
// and summed in slot order from 0, one non-temporal store of the row and one per-row maximum.  No
// size classes; no LDS and no barrier except block_amax_commit's 16 bytes and one __syncthreads,
// which run only when out_amax is asked for without out_row_amax.
//
// Narrow rows (D <= 64 floats = 16 float4 lanes) leave three quarters of such a wave idle: the
// sub-wave form gives every 16-lane group of a wave a row of its own (four rows per wave), the
// ids on the group's lanes 16 per chunk and broadcast inside the group.  Both forms add the same
// products in the same order with pinned roundings (fmaf / fmul / fadd, never contracted by the
// compiler), so a row's bits do not depend on the form, the instance, the chunking or the batch
// it is computed in.  MVML_OPT_GCN_SUBWAVE picks the form for D <= 64.
#include "gat_agg_common.h"

namespace mvml {
namespace {

__device__ __forceinline__ float4 fma4_rn(float a, float4 x, float4 c) {
  return make_float4(__fmaf_rn(a, x.x, c.x), __fmaf_rn(a, x.y, c.y), __fmaf_rn(a, x.z, c.z),
                     __fmaf_rn(a, x.w, c.w));
}
__device__ __forceinline__ float relu(float x) { return x > 0.f ? x : 0.f; }
// act(rs * acc + b): one multiply and one add per element, each rounded once
__device__ __forceinline__ float4 gcn_epilogue(float4 acc, float rs, float4 b, int act) {
  float4 o = make_float4(__fadd_rn(__fmul_rn(rs, acc.x), b.x), __fadd_rn(__fmul_rn(rs, acc.y), b.y),
                         __fadd_rn(__fmul_rn(rs, acc.z), b.z), __fadd_rn(__fmul_rn(rs, acc.w), b.w));
  if (act) o = make_float4(relu(o.x), relu(o.y), relu(o.z), relu(o.w));
  return o;
}

// One wave per row; NJ float4 column slots per lane, U neighbour rows in flight.
template <int NJ, int U>
__global__ void __launch_bounds__(256)
gcn_agg_row_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
                   const float* __restrict__ X, int64_t ldx, int D, const float* __restrict__ nbr_scale,
                   const float* __restrict__ row_scale, const float* __restrict__ bias, int act,
                   float* __restrict__ out, int64_t ldo, uint32_t* __restrict__ out_amax,
                   uint32_t* __restrict__ out_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t v = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float omx = 0.f;
  if (v < N) {  // (no early return: block_amax_commit below has a barrier)
    bool ok[NJ];
    float4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      ok[j] = 4 * (lane + 64 * j) < D;
      acc[j] = f4(0.f);
    }
    const int eb = rowptr[v], deg = rowptr[v + 1] - eb;
    for (int base = 0; base < deg; base += 64) {  // more than 64 entries (hubs): more chunks
      const int cnt = min(64, deg - base);
      const int id_l = lane < cnt ? nbr[eb + base + lane] : 0;
      const float w_l = (nbr_scale && lane < cnt) ? nbr_scale[id_l] : 1.f;
      for (int j0 = 0; j0 < cnt; j0 += U) {
        float4 x[U][NJ];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = min(j0 + u, cnt - 1);  // past the chunk: a duplicate row, not summed
          const float* xr = X + (int64_t)rl(id_l, e) * ldx;
#pragma unroll
          for (int j = 0; j < NJ; ++j) x[u][j] = ok[j] ? ld4(xr + 4 * (lane + 64 * j)) : f4(0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (j0 + u < cnt) {  // (uniform)
            const float w = rl(w_l, j0 + u);
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = fma4_rn(w, x[u][j], acc[j]);
          }
        }
      }
    }
    const float rs = row_scale ? row_scale[v] : 1.f;
    float rmx = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (!ok[j]) continue;
      const int c = 4 * (lane + 64 * j);
      const float4 o = gcn_epilogue(acc[j], rs, bias ? ld4(bias + c) : f4(0.f), act);
      st4nt(out + v * ldo + c, o);
      rmx = amax4(rmx, o);
    }
    omx = wave_max(rmx);
    if (out_rows && lane == 0) out_rows[v] = __float_as_uint(omx);
  }
  if (out_amax) block_amax_commit<256>(omx, out_amax);
}

// Sub-wave form, D <= 64: each 16-lane group of a wave owns one row (16 rows per workgroup), lane
// s of a group the float4 column s.  The chunk loops run to the wave's longest row; a group past
// its own row's end loads and adds nothing.
template <int U>
__global__ void __launch_bounds__(256)
gcn_agg_sub_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
                   const float* __restrict__ X, int64_t ldx, int D, const float* __restrict__ nbr_scale,
                   const float* __restrict__ row_scale, const float* __restrict__ bias, int act,
                   float* __restrict__ out, int64_t ldo, uint32_t* __restrict__ out_amax,
                   uint32_t* __restrict__ out_rows) {
  const int lane = threadIdx.x & 63, sl = lane & 15, g0 = lane & 48;
  const int64_t v = (xcd_block(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const bool row = v < N;
  const bool ok = row && 4 * sl < D;
  // the maximum over the wave's four groups of a value that is uniform inside each group
  auto groups_max = [](int x) {
    x = max(x, __shfl_xor(x, 16, 64));
    return max(x, __shfl_xor(x, 32, 64));
  };
  int eb = 0, deg = 0;
  if (row) {
    eb = rowptr[v];
    deg = rowptr[v + 1] - eb;
  }
  const int mdeg = groups_max(deg);
  float4 acc = f4(0.f);
  for (int base = 0; base < mdeg; base += 16) {
    const int cnt = max(0, min(16, deg - base));
    const int id_l = sl < cnt ? nbr[eb + base + sl] : 0;
    const float w_l = (nbr_scale && sl < cnt) ? nbr_scale[id_l] : 1.f;
    const int mcnt = groups_max(cnt);
    for (int j0 = 0; j0 < mcnt; j0 += U) {
      float4 x[U];
      float w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = g0 + min(j0 + u, 15);
        const int id = __shfl(id_l, e, 64);
        w[u] = __shfl(w_l, e, 64);
        x[u] = (ok && j0 + u < cnt) ? ld4(X + (int64_t)id * ldx + 4 * sl) : f4(0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j0 + u < cnt) acc = fma4_rn(w[u], x[u], acc);
    }
  }
  float rmx = 0.f;
  if (ok) {
    const float rs = row_scale ? row_scale[v] : 1.f;
    const float4 o = gcn_epilogue(acc, rs, bias ? ld4(bias + 4 * sl) : f4(0.f), act);
    st4nt(out + v * ldo + 4 * sl, o);
    rmx = amax4(rmx, o);
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) rmx = fmaxf(rmx, __shfl_xor(rmx, o, 64));  // the group's row
  if (out_rows && row && sl == 0) out_rows[v] = __float_as_uint(rmx);
  if (out_amax) block_amax_commit<256>(rmx, out_amax);
}

// One thread per node: GraphConv's factors from the degrees (clamped to >= 1, as dgl does),
// rounded once from double.
__global__ void __launch_bounds__(256)
gcn_norm_scales_kernel(int64_t N, const int32_t* __restrict__ in_rowptr, const int32_t* __restrict__ out_rowptr,
                       int norm, float* __restrict__ src_scale, float* __restrict__ dst_scale) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  float s = 1.f, d = 1.f;
  if (norm == 1 || norm == 2) {
    const double deg = (double)max(in_rowptr[v + 1] - in_rowptr[v], 1);
    d = (float)(norm == 1 ? 1.0 / sqrt(deg) : 1.0 / deg);
  }
  if (norm == 1 || norm == 3) {
    const double deg = (double)max(out_rowptr[v + 1] - out_rowptr[v], 1);
    s = (float)(norm == 1 ? 1.0 / sqrt(deg) : 1.0 / deg);
  }
  src_scale[v] = s;
  dst_scale[v] = d;
}

// Neighbour rows in flight per wave of the one-row form, by column slots per lane (the
// destination-wave GAT forward's measured choice: fewer rows, more waves, from three slots on).
constexpr int gcn_rows_in_flight(int NJ) { return NJ <= 2 ? 4 : 2; }

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_gcn_agg(int64_t num_nodes, const int32_t* rowptr, const int32_t* nbr, const float* X,
                            int64_t ldx, int D, const float* nbr_scale, const float* row_scale,
                            const float* bias, int act, float* out, int64_t ldo, uint32_t* out_amax,
                            uint32_t* out_row_amax, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "gcn_agg: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "gcn_agg: D must be a positive multiple of 4 <= 2048 (got %d)", D);
  MVML_REQUIRE(act == 0 || act == 1, "gcn_agg: bad act %d", act);
  MVML_REQUIRE(rowptr != nullptr && nbr != nullptr, "gcn_agg: rowptr and nbr are required");
  MVML_REQUIRE(row_ok(X, ldx, D) && row_ok(out, ldo, D),
               "gcn_agg: X and out must be 16-byte aligned with row strides ldx, ldo >= D that are multiples of 4");
  MVML_REQUIRE(aligned16(bias), "gcn_agg: bias must be 16-byte aligned");
  if (num_nodes == 0) return MVML_OK;
  {  // the address ranges of X's and out's rows must not meet (a wave reads rows others store)
    const float *xe = X + (num_nodes - 1) * ldx + D, *oe = out + (num_nodes - 1) * ldo + D;
    MVML_REQUIRE(oe <= X || xe <= out, "gcn_agg: out must not alias X");
  }
  const hipStream_t st = as_stream(stream);
  // with per-row maxima requested, max |out| comes from them afterwards (no per-block atomics)
  uint32_t* blk_amax = out_row_amax ? nullptr : out_amax;
  if (D <= 64 && option(MVML_OPT_GCN_SUBWAVE) != 0) {
    gcn_agg_sub_kernel<4><<<(unsigned)ceil_div(num_nodes, 16), 256, 0, st>>>(
        num_nodes, rowptr, nbr, X, ldx, D, nbr_scale, row_scale, bias, act, out, ldo, blk_amax, out_row_amax);
  } else {
    const int nj = (int)ceil_div(D / 4, 64);
    switch_const<1, 2, 3, 4, 8>(nj <= 4 ? nj : 8, [&](auto s) {
      constexpr int NJ = decltype(s)::value;
      gcn_agg_row_kernel<NJ, gcn_rows_in_flight(NJ)><<<(unsigned)ceil_div(num_nodes, 4), 256, 0, st>>>(
          num_nodes, rowptr, nbr, X, ldx, D, nbr_scale, row_scale, bias, act, out, ldo, blk_amax, out_row_amax);
      return MVML_OK;
    });
  }
  if (int rc = check_launch("gcn_agg_kernel")) return rc;
  return launch_rows_amax(num_nodes, out_row_amax, out_amax, st);
}

extern "C" int mvml_gcn_norm_scales(int64_t num_nodes, const int32_t* in_rowptr, const int32_t* out_rowptr,
                                    int norm, float* src_scale, float* dst_scale, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "gcn_norm_scales: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(norm >= 0 && norm <= 3, "gcn_norm_scales: norm must be 0 (none), 1 (both), 2 (right) or 3 (left), got %d",
               norm);
  MVML_REQUIRE(src_scale != nullptr && dst_scale != nullptr, "gcn_norm_scales: both outputs are required");
  MVML_REQUIRE((in_rowptr != nullptr || norm == 0 || norm == 3) && (out_rowptr != nullptr || norm == 0 || norm == 2),
               "gcn_norm_scales: norm %d needs the row pointers of the degrees it reads", norm);
  if (num_nodes == 0) return MVML_OK;
  gcn_norm_scales_kernel<<<(unsigned)ceil_div(num_nodes, 256), 256, 0, as_stream(stream)>>>(
      num_nodes, in_rowptr, out_rowptr, norm, src_scale, dst_scale);
  return check_launch("gcn_norm_scales_kernel");
}
