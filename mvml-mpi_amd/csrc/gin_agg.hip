// GIN's edge-aware aggregation and the embedding tables around it (dgllife 0.3.0 gnn/gin.py:
// GINLayer.forward's update_all(u_add_e, sum) over categorical bond features, GIN.forward's summed
// atom embeddings; restated, parity with dgllife unpinned).
//
//   codes:  code[s] = byte t -> off_t + cat_t[in_eid[s]]            one int32 per in-CSR slot
//   fwd:    out[v]  = sum_s (X[in_src[s]] + (E[row_0(s)] + E[row_1(s)] + ...))   s over v's in-CSR row
//   dE:     dE[r]   = sum_v cnt_r(v) * G[v]       cnt_r(v) = in-slots of v whose code names row r
//   embed:  out[n]  = sum_t Tab[off_t + idx_t[n]];   dTab[r] = sum_{n: some idx_t[n] names r} G[n]
//
// (The input gradient of the sum, dX[u] = sum over out-edges of g[dst], is mvml_gcn_agg over the
// out-CSR with NULL scales.)
//
// The forward has gcn_agg_row_kernel's form (gcn_agg.hip): one wave per row, lanes on the float4
// columns c = lane + 64 j with the last slot masked, ids and codes loaded 64 per chunk onto the
// lanes and broadcast by readlane, whole neighbour rows gathered into registers (U in flight), one
// non-temporal store per row.  Every add is an __fadd_rn in a fixed order (the edge term in table
// order, then x + e, then onto the running sum in slot order from 0), so a row's bits depend on
// neither the instance, the chunking, the table path nor the batch.  The concatenated tables E
// ([R][lde], R <= 256) are read by every wave: where R * D floats fit kGinLdsBytes a workgroup
// stages them in LDS once and then walks kGinRowsPerWave rows per wave; otherwise (or with
// MVML_OPT_GIN_LDS = 0) each wave reads the table rows it needs from L2, one row per wave.
// Narrow rows (D <= 64) run four to a wave in the sub-wave form, bitwise the one-row form;
// MVML_OPT_GIN_SUBWAVE picks the form for D <= 64.
//
// The two table gradients are two-stage sums without atomics: mvml_gin_partial_rows(N) partial
// tables, each over a contiguous atom range in ascending atom order, then mvml_colsum_f32 over the
// [P][R * D] matrix.  Stage one is a grid of (atom range) x (group of 8 table rows) x (256-column
// chunk); a wave keeps its 8 rows' accumulators in registers, counts its rows' occurrences for 64
// atoms at a time (one atom per lane) and reads a G row only when one of its rows occurs there.  A
// popular row (carbon) is therefore spread over every atom range, never summed by one wave.
#include "gat_agg_common.h"

namespace mvml {
namespace {

constexpr int kGinMaxTables = 4;
constexpr int kGinMaxRows = 256;          // edge rows over all tables: one byte per table in a code
constexpr int kEmbMaxRows = 128;          // rows of one node table
constexpr int kGinLdsBytes = 48 * 1024;   // staged tables: three workgroups per CU keep theirs
constexpr int kGinRowsPerWave = 8;        // rows a wave walks per staged copy
constexpr int kGroupRows = 8;             // table rows per wave of the gradient's first stage

// T category arrays, their table sizes and the tables' first rows in the concatenated table
struct Cats {
  const int32_t* p[kGinMaxTables];
  int n[kGinMaxTables];
  int off[kGinMaxTables];
  int T;
};

__device__ __forceinline__ float4 add4_rn(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float4 fma4_rn(float a, float4 x, float4 c) {
  return make_float4(__fmaf_rn(a, x.x, c.x), __fmaf_rn(a, x.y, c.y), __fmaf_rn(a, x.z, c.z),
                     __fmaf_rn(a, x.w, c.w));
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// category c of table t as a row of the concatenated table, clamped into the table; *bad counts
// the categories outside [0, n_t)
__device__ __forceinline__ int table_row(const Cats& cs, int t, int c, int* bad) {
  const bool out = c < 0 || c >= cs.n[t];
  *bad += out ? 1 : 0;
  return cs.off[t] + min(max(c, 0), cs.n[t] - 1);
}

// One thread per in-CSR slot.
__global__ void __launch_bounds__(256)
gin_edge_codes_kernel(int64_t E, Cats cs, const int32_t* __restrict__ in_eid, int32_t* __restrict__ codes,
                      int32_t* __restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int bad = 0;
  if (s < E) {
    int eid = in_eid[s];
    if (eid < 0 || eid >= E) {  // not an index of mvml_build_csr: counted, read as edge 0
      ++bad;
      eid = 0;
    }
    uint32_t code = 0;
#pragma unroll
    for (int t = 0; t < kGinMaxTables; ++t)
      if (t < cs.T) code |= (uint32_t)table_row(cs, t, cs.p[t][eid], &bad) << (8 * t);
    codes[s] = (int32_t)code;
  }
  bad = wave_sum_i(bad);
  if (bad && (threadIdx.x & 63) == 0) atomicAdd(status, bad);
}

// One wave per row (LDS: kGinRowsPerWave consecutive rows); NJ float4 column slots per lane, U
// neighbour rows in flight.
template <int NJ, int U, bool LDS>
__global__ void __launch_bounds__(256)
gin_agg_fwd_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
                   const int32_t* __restrict__ codes, const float* __restrict__ X, int64_t ldx, int D,
                   const float* __restrict__ Etab, int64_t lde, int R, int T, float* __restrict__ out,
                   int64_t ldo, uint32_t* __restrict__ out_amax, uint32_t* __restrict__ out_rows) {
  extern __shared__ float4 s_tab[];  // LDS: [R][D / 4]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = D / 4;
  if (LDS) {
    for (int i = threadIdx.x; i < R * q; i += 256) {
      const int r = i / q;
      s_tab[i] = ld4(Etab + (int64_t)r * lde + 4 * (i - r * q));
    }
    __syncthreads();
  }
  constexpr int RPW = LDS ? kGinRowsPerWave : 1;
  const int64_t v0 = (xcd_block(blockIdx.x, gridDim.x) * 4 + wave) * RPW;
  bool ok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) ok[j] = 4 * (lane + 64 * j) < D;
  // row r of the tables at this lane's column slot j
  auto tab = [&](int r, int j) {
    if (!ok[j]) return f4(0.f);
    return LDS ? s_tab[r * q + lane + 64 * j] : ld4(Etab + (int64_t)r * lde + 4 * (lane + 64 * j));
  };
  for (int i = 0; i < RPW; ++i) {
    const int64_t v = v0 + i;
    if (v >= N) break;  // (uniform; no barrier below)
    float4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f4(0.f);
    const int eb = rowptr[v], deg = rowptr[v + 1] - eb;
    for (int base = 0; base < deg; base += 64) {  // more than 64 entries (hubs): more chunks
      const int cnt = min(64, deg - base);
      const int id_l = lane < cnt ? nbr[eb + base + lane] : 0;
      const int code_l = lane < cnt ? codes[eb + base + lane] : 0;
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
            const uint32_t code = (uint32_t)rl(code_l, j0 + u);
            // a byte past the tables cannot come from mvml_gin_edge_codes: clamped all the same
            const int r0 = min((int)(code & 255u), R - 1);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
              float4 e = tab(r0, j);
#pragma unroll
              for (int t = 1; t < kGinMaxTables; ++t)
                if (t < T) e = add4_rn(e, tab(min((int)((code >> (8 * t)) & 255u), R - 1), j));
              acc[j] = add4_rn(acc[j], add4_rn(x[u][j], e));
            }
          }
        }
      }
    }
    float rmx = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (!ok[j]) continue;
      const int c = 4 * (lane + 64 * j);
      st4nt(out + v * ldo + c, acc[j]);
      rmx = amax4(rmx, acc[j]);
    }
    rmx = wave_max(rmx);
    if (lane == 0) {
      if (out_rows) out_rows[v] = __float_as_uint(rmx);
      if (out_amax) atomicMax(out_amax, __float_as_uint(rmx));  // unsigned bits: order-independent
    }
  }
}

// Sub-wave form, D <= 64 (gcn_agg_sub_kernel's shape): each 16-lane group of a wave owns one row,
// lane s of a group the float4 column s, ids and codes on the group's lanes 16 per chunk.  The
// chunk loops run to the wave's longest row; a group past its own row's end loads and adds
// nothing.  The same additions in the same order as the one-row form: the same bits.
__device__ __forceinline__ int groups_max(int x) {  // over a wave's four groups, x uniform in each
  x = max(x, __shfl_xor(x, 16, 64));
  return max(x, __shfl_xor(x, 32, 64));
}

template <int U, bool LDS>
__global__ void __launch_bounds__(256)
gin_agg_fwd_sub_kernel(int64_t N, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
                       const int32_t* __restrict__ codes, const float* __restrict__ X, int64_t ldx, int D,
                       const float* __restrict__ Etab, int64_t lde, int R, int T, float* __restrict__ out,
                       int64_t ldo, uint32_t* __restrict__ out_amax, uint32_t* __restrict__ out_rows) {
  extern __shared__ float4 s_tab[];  // LDS: [R][D / 4]
  const int lane = threadIdx.x & 63, sl = lane & 15, g0 = lane & 48;
  const int q = D / 4;
  if (LDS) {
    for (int i = threadIdx.x; i < R * q; i += 256) {
      const int r = i / q;
      s_tab[i] = ld4(Etab + (int64_t)r * lde + 4 * (i - r * q));
    }
    __syncthreads();
  }
  constexpr int RPW = LDS ? kGinRowsPerWave : 1;  // groups of four rows a wave walks
  const int64_t w0 = (xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * RPW;
  const bool col = 4 * sl < D;
  auto tab = [&](uint32_t code, int t) {
    const int r = min((int)((code >> (8 * t)) & 255u), R - 1);
    if (!col) return f4(0.f);
    return LDS ? s_tab[r * q + sl] : ld4(Etab + (int64_t)r * lde + 4 * sl);
  };
  for (int i = 0; i < RPW; ++i) {
    if ((w0 + i) * 4 >= N) break;  // (uniform; no barrier below)
    const int64_t v = (w0 + i) * 4 + (lane >> 4);
    const bool row = v < N;
    const bool ok = row && col;
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
      const int code_l = sl < cnt ? codes[eb + base + sl] : 0;
      const int mcnt = groups_max(cnt);
      for (int j0 = 0; j0 < mcnt; j0 += U) {
        float4 x[U];
        uint32_t code[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = g0 + min(j0 + u, 15);
          const int id = __shfl(id_l, e, 64);
          code[u] = (uint32_t)__shfl(code_l, e, 64);
          x[u] = (ok && j0 + u < cnt) ? ld4(X + (int64_t)id * ldx + 4 * sl) : f4(0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (j0 + u < cnt) {
            float4 e = tab(code[u], 0);
#pragma unroll
            for (int t = 1; t < kGinMaxTables; ++t)
              if (t < T) e = add4_rn(e, tab(code[u], t));
            acc = add4_rn(acc, add4_rn(x[u], e));
          }
        }
      }
    }
    float rmx = 0.f;
    if (ok) {
      st4nt(out + v * ldo + 4 * sl, acc);
      rmx = amax4(rmx, acc);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) rmx = fmaxf(rmx, __shfl_xor(rmx, o, 64));  // the group's row
    if (row && sl == 0) {
      if (out_rows) out_rows[v] = __float_as_uint(rmx);
      if (out_amax) atomicMax(out_amax, __float_as_uint(rmx));
    }
  }
}

// What the gradient's first stage counts: (edge tables) the codes of an atom's in-slots, or (node
// tables) the atom's own T indices.
struct CountSrc {
  const int32_t* rowptr;
  const int32_t* codes;
  Cats cats;
};

// Wave (p, row group, column chunk): part[p][r0 .. r0 + 8)[chunk] = sum over the atoms v of range p,
// ascending, of cnt_r(v) * G[v], each step one fma.
template <bool NODE>
__global__ void __launch_bounds__(256)
emb_grad_partial_kernel(int64_t N, int64_t P, CountSrc cs, const float* __restrict__ G, int64_t ldg, int D, int R,
                        float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= P) return;
  const int r0 = blockIdx.y * kGroupRows;
  const int c = 4 * (blockIdx.z * 64 + lane);
  const bool ok = c < D;
  const int64_t per = ceil_div(N, P);
  const int64_t a0 = min(p * per, N), a1 = min(a0 + per, N);
  const int T = cs.cats.T;
  float4 acc[kGroupRows];
#pragma unroll
  for (int k = 0; k < kGroupRows; ++k) acc[k] = f4(0.f);
  for (int64_t base = a0; base < a1; base += 64) {
    const int64_t v = base + lane;
    int cnt[kGroupRows];
#pragma unroll
    for (int k = 0; k < kGroupRows; ++k) cnt[k] = 0;
    if (v < a1) {
      if (NODE) {
#pragma unroll
        for (int t = 0; t < kGinMaxTables; ++t) {
          if (t < T) {
            int bad = 0;
            const int row = table_row(cs.cats, t, cs.cats.p[t][v], &bad) - r0;
#pragma unroll
            for (int k = 0; k < kGroupRows; ++k) cnt[k] += row == k ? 1 : 0;
          }
        }
      } else {
        const int se = cs.rowptr[v + 1];
        for (int s = cs.rowptr[v]; s < se; ++s) {
          const uint32_t code = (uint32_t)cs.codes[s];
#pragma unroll
          for (int t = 0; t < kGinMaxTables; ++t) {
            if (t < T) {
              const int row = min((int)((code >> (8 * t)) & 255u), R - 1) - r0;
#pragma unroll
              for (int k = 0; k < kGroupRows; ++k) cnt[k] += row == k ? 1 : 0;
            }
          }
        }
      }
    }
    int any = 0;
#pragma unroll
    for (int k = 0; k < kGroupRows; ++k) any |= cnt[k];
    unsigned long long m = __ballot(any != 0);
    while (m) {  // (uniform) the atoms of this block of 64 that name one of the wave's rows
      const int j = __ffsll(m) - 1;
      m &= m - 1;
      const float4 g = ok ? ld4(G + (base + j) * ldg + c) : f4(0.f);
#pragma unroll
      for (int k = 0; k < kGroupRows; ++k) {
        const int ck = rl(cnt[k], j);
        if (ck) acc[k] = fma4_rn((float)ck, g, acc[k]);
      }
    }
  }
  if (ok) {
#pragma unroll
    for (int k = 0; k < kGroupRows; ++k)
      if (r0 + k < R) st4(part + ((int64_t)p * R + r0 + k) * D + c, acc[k]);
  }
}

// One thread per float4 of out.
__global__ void __launch_bounds__(256)
embed_sum_fwd_kernel(int64_t N, Cats cs, const float* __restrict__ tab, int64_t ldt, int D, float* __restrict__ out,
                     int64_t ldo, int32_t* __restrict__ status) {
  const int q = D / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * q) return;
  const int64_t v = i / q;
  const int c = 4 * (int)(i - v * q);
  int bad = 0;
  float4 o = ld4(tab + (int64_t)table_row(cs, 0, cs.p[0][v], &bad) * ldt + c);
#pragma unroll
  for (int t = 1; t < kGinMaxTables; ++t)
    if (t < cs.T) o = add4_rn(o, ld4(tab + (int64_t)table_row(cs, t, cs.p[t][v], &bad) * ldt + c));
  st4(out + v * ldo + c, o);
  if (bad && c == 0 && status) atomicAdd(status, bad);  // (one thread per atom counts)
}

// One thread per float4.
__global__ void __launch_bounds__(256)
relu_f32_kernel(int64_t n4, int64_t n, const float* __restrict__ x, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) {
    const float4 a = ld4(x + 4 * i);
    st4(y + 4 * i, make_float4(a.x > 0.f ? a.x : 0.f, a.y > 0.f ? a.y : 0.f, a.z > 0.f ? a.z : 0.f,
                               a.w > 0.f ? a.w : 0.f));
  } else if (i == n4) {  // the tail of a length that is no multiple of 4
    for (int64_t k = 4 * n4; k < n; ++k) y[k] = x[k] > 0.f ? x[k] : 0.f;
  }
}

constexpr int gin_rows_in_flight(int NJ) { return NJ <= 2 ? 4 : 2; }

inline bool ranges_meet(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const char *a0 = (const char*)a, *b0 = (const char*)b;
  return !(a0 + abytes <= b0 || b0 + bbytes <= a0);
}
inline int64_t rows_bytes(int64_t n, int64_t ld, int D) { return 4 * ((n - 1) * ld + D); }

// The T tables of an entry point: sizes in [1, max_rows], pointers present, T in [1, 4]; fills
// the offsets and returns the total row count, or -1.
inline int fill_cats(Cats* cs, int T, const int32_t* c0, const int32_t* c1, const int32_t* c2, const int32_t* c3,
                     int n0, int n1, int n2, int n3, int max_rows, bool need_ptrs) {
  if (T < 1 || T > kGinMaxTables) return -1;
  const int32_t* p[4] = {c0, c1, c2, c3};
  const int n[4] = {n0, n1, n2, n3};
  int off = 0;
  for (int t = 0; t < kGinMaxTables; ++t) {
    cs->p[t] = t < T ? p[t] : nullptr;
    cs->n[t] = t < T ? n[t] : 1;
    cs->off[t] = t < T ? off : 0;
    if (t < T) {
      if (n[t] < 1 || n[t] > max_rows || (need_ptrs && p[t] == nullptr)) return -1;
      off += n[t];
    }
  }
  cs->T = T;
  return off;
}

template <bool NODE>
int emb_grad(const char* who, int64_t N, const CountSrc& cs, const float* G, int64_t ldg, int D, int R, float* dE,
             void* workspace, size_t workspace_bytes, hipStream_t st) {
  const int64_t P = mvml_gin_partial_rows(N);
  const size_t need = mvml_gin_emb_grad_workspace_size(N, R, D);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  Carver cv(workspace, workspace_bytes);
  float* part = cv.take<float>((size_t)P * R * D);
  void* cws = cv.take<char>(mvml_colsum_workspace_size(P, (int64_t)R * D));
  const dim3 grid((unsigned)ceil_div(P, 4), (unsigned)ceil_div(R, kGroupRows), (unsigned)ceil_div(D, 256));
  emb_grad_partial_kernel<NODE><<<grid, 256, 0, st>>>(N, P, cs, G, ldg, D, R, part);
  if (int rc = check_launch("emb_grad_partial_kernel")) return rc;
  return mvml_colsum_f32(P, (int64_t)R * D, part, (int64_t)R * D, 1.f, 0.f, dE, cws,
                         mvml_colsum_workspace_size(P, (int64_t)R * D), st);
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_gin_edge_codes(int64_t num_edges, int T, const int32_t* cat0, const int32_t* cat1,
                                   const int32_t* cat2, const int32_t* cat3, int n0, int n1, int n2, int n3,
                                   const int32_t* in_eid, int32_t* codes, int32_t* status, void* stream) {
  clear_error();
  MVML_REQUIRE(num_edges >= 0 && num_edges < (int64_t(1) << 31), "gin_edge_codes: bad num_edges %lld",
               (long long)num_edges);
  Cats cs;
  const int R = fill_cats(&cs, T, cat0, cat1, cat2, cat3, n0, n1, n2, n3, kGinMaxRows, num_edges > 0);
  MVML_REQUIRE(R > 0 && R <= kGinMaxRows,
               "gin_edge_codes: 1 to 4 tables of at least one row each, at most 256 rows in all, a category "
               "array per table");
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(in_eid != nullptr && codes != nullptr && status != nullptr,
               "gin_edge_codes: in_eid, codes and status are required");
  gin_edge_codes_kernel<<<(unsigned)ceil_div(num_edges, 256), 256, 0, as_stream(stream)>>>(num_edges, cs, in_eid,
                                                                                         codes, status);
  return check_launch("gin_edge_codes_kernel");
}

extern "C" int mvml_gin_agg_fwd(int64_t num_nodes, const int32_t* in_rowptr, const int32_t* in_src,
                                const int32_t* codes, const float* X, int64_t ldx, int D, const float* E,
                                int64_t lde, int R, int T, float* out, int64_t ldo, uint32_t* out_amax,
                                uint32_t* out_row_amax, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "gin_agg_fwd: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024, "gin_agg_fwd: D must be a positive multiple of 4 <= 1024 (got %d)", D);
  MVML_REQUIRE(R >= 1 && R <= kGinMaxRows && T >= 1 && T <= kGinMaxTables && T <= R,
               "gin_agg_fwd: 1 <= T <= 4 tables of 1 <= R <= 256 rows in all (got T = %d, R = %d)", T, R);
  MVML_REQUIRE(in_rowptr != nullptr && in_src != nullptr && codes != nullptr,
               "gin_agg_fwd: in_rowptr, in_src and codes are required");
  MVML_REQUIRE(row_ok(X, ldx, D) && row_ok(out, ldo, D) && row_ok(E, lde, D),
               "gin_agg_fwd: X, out and E must be 16-byte aligned with row strides >= D that are multiples of 4");
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(!ranges_meet(X, rows_bytes(num_nodes, ldx, D), out, rows_bytes(num_nodes, ldo, D)) &&
                   !ranges_meet(E, rows_bytes(R, lde, D), out, rows_bytes(num_nodes, ldo, D)),
               "gin_agg_fwd: out must not alias X or E");
  const hipStream_t st = as_stream(stream);
  uint32_t* blk_amax = out_row_amax ? nullptr : out_amax;
  const size_t tab_bytes = (size_t)R * D * 4;
  const bool lds = option(MVML_OPT_GIN_LDS) != 0 && tab_bytes <= (size_t)kGinLdsBytes;
  const int nj = (int)ceil_div(D / 4, 64);
  if (D <= 64 && option(MVML_OPT_GIN_SUBWAVE) != 0) {
    if (lds)
      gin_agg_fwd_sub_kernel<4, true><<<(unsigned)ceil_div(num_nodes, 16 * kGinRowsPerWave), 256, tab_bytes, st>>>(
          num_nodes, in_rowptr, in_src, codes, X, ldx, D, E, lde, R, T, out, ldo, blk_amax, out_row_amax);
    else
      gin_agg_fwd_sub_kernel<4, false><<<(unsigned)ceil_div(num_nodes, 16), 256, 0, st>>>(
          num_nodes, in_rowptr, in_src, codes, X, ldx, D, E, lde, R, T, out, ldo, blk_amax, out_row_amax);
  } else switch_const<1, 2, 3, 4>(nj, [&](auto s) {
    constexpr int NJ = decltype(s)::value;
    constexpr int U = gin_rows_in_flight(NJ);
    if (lds)
      gin_agg_fwd_kernel<NJ, U, true><<<(unsigned)ceil_div(num_nodes, 4 * kGinRowsPerWave), 256, tab_bytes, st>>>(
          num_nodes, in_rowptr, in_src, codes, X, ldx, D, E, lde, R, T, out, ldo, blk_amax, out_row_amax);
    else
      gin_agg_fwd_kernel<NJ, U, false><<<(unsigned)ceil_div(num_nodes, 4), 256, 0, st>>>(
          num_nodes, in_rowptr, in_src, codes, X, ldx, D, E, lde, R, T, out, ldo, blk_amax, out_row_amax);
    return MVML_OK;
  });
  if (int rc = check_launch("gin_agg_fwd_kernel")) return rc;
  return launch_rows_amax(num_nodes, out_row_amax, out_amax, st);
}

extern "C" int64_t mvml_gin_partial_rows(int64_t num_nodes) {
  return std::min<int64_t>(std::max<int64_t>(ceil_div(num_nodes, 128), 1), 2048);
}

extern "C" size_t mvml_gin_emb_grad_workspace_size(int64_t num_nodes, int R, int D) {
  if (num_nodes < 0 || R <= 0 || D <= 0) return 0;
  const int64_t P = mvml_gin_partial_rows(num_nodes);
  return carve_size((size_t)P * R * D * 4) + carve_size(mvml_colsum_workspace_size(P, (int64_t)R * D)) + 256;
}

extern "C" int mvml_gin_edge_emb_grad(int64_t num_nodes, const int32_t* in_rowptr, const int32_t* codes,
                                      const float* G, int64_t ldg, int D, int R, int T, float* dE,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "gin_edge_emb_grad: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024,
               "gin_edge_emb_grad: D must be a positive multiple of 4 <= 1024 (got %d)", D);
  MVML_REQUIRE(R >= 1 && R <= kGinMaxRows && T >= 1 && T <= kGinMaxTables && T <= R,
               "gin_edge_emb_grad: 1 <= T <= 4 tables of 1 <= R <= 256 rows in all (got T = %d, R = %d)", T, R);
  MVML_REQUIRE(dE != nullptr && aligned16(dE), "gin_edge_emb_grad: dE is required, 16-byte aligned");
  const hipStream_t st = as_stream(stream);
  if (num_nodes == 0) return mvml_fill_zero(dE, 1, (int64_t)R * D * 4, (int64_t)R * D * 4, stream);
  MVML_REQUIRE(in_rowptr != nullptr && codes != nullptr, "gin_edge_emb_grad: in_rowptr and codes are required");
  MVML_REQUIRE(row_ok(G, ldg, D), "gin_edge_emb_grad: G must be 16-byte aligned with a row stride >= D that is a multiple of 4");
  MVML_REQUIRE(!ranges_meet(G, rows_bytes(num_nodes, ldg, D), dE, (int64_t)R * D * 4),
               "gin_edge_emb_grad: dE must not alias G");
  CountSrc cs{};
  cs.rowptr = in_rowptr;
  cs.codes = codes;
  cs.cats.T = T;
  return emb_grad<false>("gin_edge_emb_grad", num_nodes, cs, G, ldg, D, R, dE, workspace, workspace_bytes, st);
}

extern "C" int mvml_embed_sum_fwd(int64_t num_nodes, int T, const int32_t* idx0, const int32_t* idx1,
                                  const int32_t* idx2, const int32_t* idx3, int n0, int n1, int n2, int n3,
                                  const float* tab, int64_t ldt, int D, float* out, int64_t ldo, int32_t* status,
                                  void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "embed_sum_fwd: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024, "embed_sum_fwd: D must be a positive multiple of 4 <= 1024 (got %d)", D);
  Cats cs;
  const int R = fill_cats(&cs, T, idx0, idx1, idx2, idx3, n0, n1, n2, n3, kEmbMaxRows, num_nodes > 0);
  MVML_REQUIRE(R > 0, "embed_sum_fwd: 1 to 4 tables of 1 to 128 rows each, an index array per table");
  MVML_REQUIRE(row_ok(tab, ldt, D) && row_ok(out, ldo, D),
               "embed_sum_fwd: tab and out must be 16-byte aligned with row strides >= D that are multiples of 4");
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(!ranges_meet(tab, rows_bytes(R, ldt, D), out, rows_bytes(num_nodes, ldo, D)),
               "embed_sum_fwd: out must not alias tab");
  embed_sum_fwd_kernel<<<(unsigned)ceil_div(num_nodes * (D / 4), 256), 256, 0, as_stream(stream)>>>(
      num_nodes, cs, tab, ldt, D, out, ldo, status);
  return check_launch("embed_sum_fwd_kernel");
}

extern "C" int mvml_embed_sum_bwd(int64_t num_nodes, int T, const int32_t* idx0, const int32_t* idx1,
                                  const int32_t* idx2, const int32_t* idx3, int n0, int n1, int n2, int n3,
                                  const float* G, int64_t ldg, int D, float* dtab, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  clear_error();
  MVML_REQUIRE(num_nodes >= 0 && num_nodes < (int64_t(1) << 31), "embed_sum_bwd: bad num_nodes %lld",
               (long long)num_nodes);
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024, "embed_sum_bwd: D must be a positive multiple of 4 <= 1024 (got %d)", D);
  CountSrc cs{};
  const int R = fill_cats(&cs.cats, T, idx0, idx1, idx2, idx3, n0, n1, n2, n3, kEmbMaxRows, num_nodes > 0);
  MVML_REQUIRE(R > 0, "embed_sum_bwd: 1 to 4 tables of 1 to 128 rows each, an index array per table");
  MVML_REQUIRE(dtab != nullptr && aligned16(dtab), "embed_sum_bwd: dtab is required, 16-byte aligned");
  if (num_nodes == 0) return mvml_fill_zero(dtab, 1, (int64_t)R * D * 4, (int64_t)R * D * 4, stream);
  MVML_REQUIRE(row_ok(G, ldg, D), "embed_sum_bwd: G must be 16-byte aligned with a row stride >= D that is a multiple of 4");
  MVML_REQUIRE(!ranges_meet(G, rows_bytes(num_nodes, ldg, D), dtab, (int64_t)R * D * 4),
               "embed_sum_bwd: dtab must not alias G");
  return emb_grad<true>("embed_sum_bwd", num_nodes, cs, G, ldg, D, R, dtab, workspace, workspace_bytes,
                        as_stream(stream));
}

extern "C" int mvml_relu_f32(int64_t n, const float* x, float* y, void* stream) {
  clear_error();
  MVML_REQUIRE(n >= 0, "relu_f32: bad n %lld", (long long)n);
  if (n == 0) return MVML_OK;
  MVML_REQUIRE(x != nullptr && y != nullptr && aligned16(x) && aligned16(y),
               "relu_f32: x and y are required, 16-byte aligned");
  const int64_t n4 = n / 4;
  relu_f32_kernel<<<(unsigned)ceil_div(n4 + 1, 256), 256, 0, as_stream(stream)>>>(n4, n, x, y);
  return check_launch("relu_f32_kernel");
}
