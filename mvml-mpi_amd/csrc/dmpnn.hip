// D-MPNN (Chemprop v1 MPNEncoder, bond messages, directed, ReLU; restated, parity with Chemprop
// unpinned): the hidden state lives on the DIRECTED BONDS.  For a bond s = (u -> v)
//
//   input_s = W_i [x_u ; e_s] (+ b_i)        M^0_s = relu(input_s)
//   M^t_s   = relu(input_s + W_h (sum_{k -> u} M^{t-1}_k - M^{t-1}_{rev(s)}) (+ b_h))
//
// Every [E, D] state is kept in in-CSR SLOT order, so the states of the bonds entering an atom are
// one contiguous block of rows.  Both products are re-associated: P = x W_ia^T is a GEMM over the N
// atom rows and R = M^{t-1} W_h^T one over the E slot rows (no gather in either), and the kernels
// here do what is left, all fp32, every add rounded once in a fixed order, no float atomics:
//
//   rev_slots  rev_slot[s] of s = (u -> v), the k-th slot of row v with source u: the k-th slot of row
//              u with source v (slots of a row are in edge-id order, so k counts in edge-id order); a
//              self-loop is its own reverse; -1 where row u has no such slot.  One thread per slot.
//   init_fwd   input[s] = (P[u] + b_i) + e_s[0] W_ieT[0] + e_s[1] W_ieT[1] + ... and M0[s] = relu of the
//              same registers.  A group of LW lanes owns a slot, lane l the float4 columns l + LW j;
//              W_ieT ([De][D]) is staged in LDS once per workgroup where it fits kDmLdsBytes (each
//              group then walks kDmRows slots), else read from L2: the same fmas either way.
//   update     for an atom v: Q = the sum of the rows of list A, then for every row f of list B
//              out[f] = Q - X[rev(f)] (nothing subtracted where rev(f) = -1).  Forward: A = v's in-slots
//              (a row range, no index list), B = v's out-edges (out_inslot), X = R, and the store is
//              relu((input[f] + b_h) + (Q - R[rev(f)])).  Adjoint: the two lists swapped, X = dpre =
//              g_out * (out > 0) formed on load and stored once (by the atom whose out-edge the slot
//              is), dR[f] = Q - dpre[rev(f)].  rev(f) of a B row is an A row: the wave has just read it.
//              One wave per atom (D <= 64: 16 lanes per atom, four atoms per wave), Q in registers,
//              16-byte accesses; lists longer than the lane group are walked in chunks, so a hub
//              needs no LDS and no second kernel.  Columns are independent: widths past 256 repeat the
//              walk per 256-column chunk.
//   atom_sum   a_v = the sum of v's in-slot rows, and its adjoint dM[s] = g_a[dst(s)]: the update
//              template with one list empty, Q stored to (or taken from) the atom's row.  Not
//              mvml_gcn_agg with an index list: its alias check takes X and out to have the same
//              number of rows, which an [E] against an [N] matrix does not.
#include "gat_agg_common.h"

namespace mvml {
namespace {

constexpr int kDmMaxDe = 32;
constexpr int kDmMaxD = 1024;
constexpr int kDmLdsBytes = 48 * 1024;  // staged W_ieT: three workgroups per CU keep theirs
constexpr int kDmRows = 8;              // slots a lane group walks per staged copy
constexpr int kDmSubD = 64;             // D <= 64: 16 lanes per row, four rows per wave

__device__ __forceinline__ float4 add4_rn(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float4 sub4_rn(float4 a, float4 b) {
  return make_float4(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z), __fsub_rn(a.w, b.w));
}
__device__ __forceinline__ float4 fma4_rn(float a, float4 x, float4 c) {
  return make_float4(__fmaf_rn(a, x.x, c.x), __fmaf_rn(a, x.y, c.y), __fmaf_rn(a, x.z, c.z),
                     __fmaf_rn(a, x.w, c.w));
}
__device__ __forceinline__ float relu(float x) { return x > 0.f ? x : 0.f; }
__device__ __forceinline__ float4 relu4(float4 q) { return make_float4(relu(q.x), relu(q.y), relu(q.z), relu(q.w)); }
// g * (o > 0): g's bits or +0, as mvml_relu_bwd
__device__ __forceinline__ float4 mask4(float4 g, float4 o) {
  return make_float4(o.x > 0.f ? g.x : 0.f, o.y > 0.f ? g.y : 0.f, o.z > 0.f ? g.z : 0.f, o.w > 0.f ? g.w : 0.f);
}
template <int LW>
__device__ __forceinline__ int groups_max(int x) {  // over a wave's lane groups, x uniform in each
  if (LW < 64) {
    x = max(x, __shfl_xor(x, 16, 64));
    x = max(x, __shfl_xor(x, 32, 64));
  }
  return x;
}
// lane e of the group that starts at lane g0 (e uniform over the wave)
template <int LW>
__device__ __forceinline__ int bcast(int x, int e, int g0) {
  return LW == 64 ? rl(x, e) : __shfl(x, g0 + e, 64);
}

// One thread per slot.
__global__ void __launch_bounds__(256)
dmpnn_rev_slots_kernel(int64_t N, int64_t E, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                       int32_t* __restrict__ rev) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= E) return;
  int64_t lo = 0, hi = N;  // the row v of slot s: rowptr[lo] <= s < rowptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid] <= s) lo = mid; else hi = mid;
  }
  const int v = (int)lo, u = src[s];
  int r = -1;
  if (u >= 0 && u < N) {  // (an id that is none of mvml_build_csr's: no reverse)
    int k = 0;
    for (int64_t i = max(rowptr[v], 0); i < s; ++i) k += src[i] == u;
    const int64_t ue = min((int64_t)rowptr[u + 1], E);
    for (int64_t i = max(rowptr[u], 0); i < ue; ++i)
      if (src[i] == v && k-- == 0) {
        r = (int)i;
        break;
      }
  }
  rev[s] = r;
}

struct DmInitArgs {
  int64_t N, E;
  const int32_t* src;
  const float* P;
  int64_t ldp;
  int D;
  const float* brows;
  int De, Dp;
  const float *WieT, *bi;
  float* inp;
  int64_t ldi;
  float* M0;
  int64_t ldm;
};

template <int LW, bool LDS>
__global__ void __launch_bounds__(256)
dmpnn_init_kernel(DmInitArgs a) {
  extern __shared__ float4 s_w[];  // LDS: [De][D / 4]
  const int q = a.D / 4;
  if (LDS) {
    for (int i = threadIdx.x; i < a.De * q; i += 256) s_w[i] = ld4(a.WieT + 4 * (int64_t)i);
    __syncthreads();
  }
  constexpr int GPB = 256 / LW;
  constexpr int RPG = LDS ? kDmRows : 1;
  const int sl = threadIdx.x & (LW - 1);
  const int64_t s0 = (xcd_block(blockIdx.x, gridDim.x) * GPB + threadIdx.x / LW) * RPG;
  const float4* w = LDS ? s_w : reinterpret_cast<const float4*>(a.WieT);
  for (int i = 0; i < RPG; ++i) {
    const int64_t s = s0 + i;
    if (s >= a.E) break;  // (no barrier and no cross-lane step below)
    int u = a.src[s];
    if (u < 0 || u >= a.N) u = 0;  // not an id of mvml_build_csr: read as atom 0
    const float* brow = a.brows + s * a.Dp;
    for (int ci = sl; ci < q; ci += LW) {
      float4 acc = add4_rn(ld4(a.P + (int64_t)u * a.ldp + 4 * ci), a.bi ? ld4(a.bi + 4 * ci) : f4(0.f));
      for (int k0 = 0; k0 < a.De; k0 += 4) {  // k ascending, one fma each
        const float4 e = ld4(brow + k0);
        acc = fma4_rn(e.x, w[(k0 + 0) * q + ci], acc);
        if (k0 + 1 < a.De) acc = fma4_rn(e.y, w[(k0 + 1) * q + ci], acc);
        if (k0 + 2 < a.De) acc = fma4_rn(e.z, w[(k0 + 2) * q + ci], acc);
        if (k0 + 3 < a.De) acc = fma4_rn(e.w, w[(k0 + 3) * q + ci], acc);
      }
      st4nt(a.inp + s * a.ldi + 4 * ci, acc);
      st4nt(a.M0 + s * a.ldm + 4 * ci, relu4(acc));
    }
  }
}

struct DmUpdArgs {
  int64_t N;
  const int32_t *a_rowptr, *a_idx;  // list A of an atom (summed); idx NULL: the row range itself
  const int32_t *b_rowptr, *b_idx;  // list B (written)
  const int32_t* rev;
  const float* X;  // forward: R; adjoint: g_out
  int64_t ldx;
  const float* Y;  // forward: input; adjoint: out (the ReLU mask)
  int64_t ldy;
  const float* bias;  // forward only, may be NULL
  int D;
  float* out;  // forward: the next state; adjoint: dR
  int64_t ldo;
  float* dpre;  // adjoint only
  int64_t ldd;
  const float* q_in;  // atom rows taken as Q in place of list A's sum (the atom sum's adjoint), or NULL
  float* q_out;       // atom rows that receive Q (the atom sum), or NULL
  int64_t ldq;
};

template <bool BWD>
__device__ __forceinline__ float4 dm_row(const DmUpdArgs& a, int s, int c) {
  const float4 x = ld4(a.X + (int64_t)s * a.ldx + c);
  return BWD ? mask4(x, ld4(a.Y + (int64_t)s * a.ldy + c)) : x;
}

// LW lanes per atom; UA rows of list A and UB rows of list B in flight.
template <int LW, bool BWD, int UA, int UB>
__global__ void __launch_bounds__(256)
dmpnn_update_kernel(DmUpdArgs a) {
  const int lane = threadIdx.x & 63, sl = lane & (LW - 1), g0 = lane & ~(LW - 1);
  const int64_t v = (xcd_block(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)) * (64 / LW) + lane / LW;
  const bool row = v < a.N;
  int ab = 0, an = 0, bb = 0, bn = 0;
  if (row) {
    if (a.a_rowptr) {
      ab = a.a_rowptr[v];
      an = a.a_rowptr[v + 1] - ab;
    }
    if (a.b_rowptr) {
      bb = a.b_rowptr[v];
      bn = a.b_rowptr[v + 1] - bb;
    }
  }
  const int man = groups_max<LW>(an), mbn = groups_max<LW>(bn);
  const int q = a.D / 4;
  for (int c0 = 0; c0 < q; c0 += LW) {  // (uniform)
    const bool ok = row && c0 + sl < q;
    const int c = 4 * (c0 + sl);
    float4 Q = (a.q_in && ok) ? ld4(a.q_in + v * a.ldq + c) : f4(0.f);
    for (int base = 0; base < man; base += LW) {  // more entries than lanes (hubs): more chunks
      const int cnt = max(0, min(LW, an - base));
      int id_l = ab + base + sl;
      if (a.a_idx) id_l = sl < cnt ? a.a_idx[id_l] : 0;
      const int mcnt = groups_max<LW>(cnt);
      for (int j0 = 0; j0 < mcnt; j0 += UA) {
        float4 x[UA];
        int s[UA];
#pragma unroll
        for (int u = 0; u < UA; ++u) {
          s[u] = bcast<LW>(id_l, min(j0 + u, LW - 1), g0);
          x[u] = (ok && j0 + u < cnt) ? dm_row<BWD>(a, s[u], c) : f4(0.f);
        }
#pragma unroll
        for (int u = 0; u < UA; ++u) {
          if (ok && j0 + u < cnt) {
            Q = add4_rn(Q, x[u]);  // list order, each add rounded once
            if (BWD) st4nt(a.dpre + (int64_t)s[u] * a.ldd + c, x[u]);
          }
        }
      }
    }
    if (a.q_out && ok) st4nt(a.q_out + v * a.ldq + c, Q);
    const float4 b = (!BWD && a.bias && ok) ? ld4(a.bias + c) : f4(0.f);
    for (int base = 0; base < mbn; base += LW) {
      const int cnt = max(0, min(LW, bn - base));
      int f_l = bb + base + sl;
      if (a.b_idx) f_l = sl < cnt ? a.b_idx[f_l] : 0;
      const int r_l = (a.rev && sl < cnt) ? a.rev[f_l] : -1;
      const int mcnt = groups_max<LW>(cnt);
      for (int j0 = 0; j0 < mcnt; j0 += UB) {
        float4 y[UB], in[UB];
        int f[UB], r[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int e = min(j0 + u, LW - 1);
          f[u] = bcast<LW>(f_l, e, g0);
          r[u] = bcast<LW>(r_l, e, g0);
          const bool live = ok && j0 + u < cnt;
          y[u] = (live && r[u] >= 0) ? dm_row<BWD>(a, r[u], c) : f4(0.f);
          in[u] = (!BWD && live) ? ld4nt(a.Y + (int64_t)f[u] * a.ldy + c) : f4(0.f);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          if (ok && j0 + u < cnt) {
            const float4 m = r[u] >= 0 ? sub4_rn(Q, y[u]) : Q;
            st4nt(a.out + (int64_t)f[u] * a.ldo + c, BWD ? m : relu4(add4_rn(add4_rn(in[u], b), m)));
          }
        }
      }
    }
  }
}

inline bool sizes_ok(int64_t N, int64_t E) {
  return N >= 0 && N < (int64_t(1) << 31) && E >= 0 && E < (int64_t(1) << 31);
}
inline bool width_ok(int D) { return D > 0 && D % 4 == 0 && D <= kDmMaxD; }
// the address ranges of two [E][ld] row blocks do not meet
inline bool apart(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t E, int D) {
  const float *pe = p + (E - 1) * ldp + D, *qe = q + (E - 1) * ldq + D;
  return pe <= q || qe <= p;
}

template <bool BWD>
int launch_update(DmUpdArgs a, hipStream_t st) {
  if (a.D <= kDmSubD)
    dmpnn_update_kernel<16, BWD, 4, 2><<<(unsigned)ceil_div(a.N, 16), 256, 0, st>>>(a);
  else
    dmpnn_update_kernel<64, BWD, 4, 2><<<(unsigned)ceil_div(a.N, 4), 256, 0, st>>>(a);
  return check_launch(BWD ? "dmpnn_update_bwd_kernel" : "dmpnn_update_kernel");
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_dmpnn_rev_slots(int64_t num_nodes, int64_t num_edges, const int32_t* in_rowptr,
                                    const int32_t* in_src, int32_t* rev_slot, void* stream) {
  clear_error();
  MVML_REQUIRE(sizes_ok(num_nodes, num_edges), "dmpnn_rev_slots: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(num_nodes > 0 && in_rowptr != nullptr && in_src != nullptr && rev_slot != nullptr,
               "dmpnn_rev_slots: in_rowptr, in_src and rev_slot are required");
  dmpnn_rev_slots_kernel<<<(unsigned)ceil_div(num_edges, 256), 256, 0, as_stream(stream)>>>(num_nodes, num_edges, in_rowptr,
                                                                                           in_src, rev_slot);
  return check_launch("dmpnn_rev_slots_kernel");
}

extern "C" int mvml_dmpnn_init_fwd(int64_t num_nodes, int64_t num_edges, const int32_t* in_src, const float* P,
                                   int64_t ldp, int D, const float* rows, int De, const float* W_ieT, const float* b_i,
                                   float* input, int64_t ldi, float* M0, int64_t ldm, void* stream) {
  clear_error();
  MVML_REQUIRE(sizes_ok(num_nodes, num_edges), "dmpnn_init_fwd: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  MVML_REQUIRE(width_ok(D), "dmpnn_init_fwd: D must be a positive multiple of 4 <= %d (got %d)", kDmMaxD, D);
  MVML_REQUIRE(De >= 1 && De <= kDmMaxDe, "dmpnn_init_fwd: 1 to %d bond features (got %d)", kDmMaxDe, De);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(num_nodes > 0 && in_src != nullptr, "dmpnn_init_fwd: in_src is required");
  MVML_REQUIRE(row_ok(P, ldp, D) && row_ok(input, ldi, D) && row_ok(M0, ldm, D),
               "dmpnn_init_fwd: P, input and M0 must be 16-byte aligned with row strides >= D that are multiples of 4");
  MVML_REQUIRE(rows != nullptr && aligned16(rows) && W_ieT != nullptr && aligned16(W_ieT) && aligned16(b_i),
               "dmpnn_init_fwd: rows, W_ieT and b_i must be 16-byte aligned (b_i may be NULL)");
  MVML_REQUIRE(apart(input, ldi, M0, ldm, num_edges, D), "dmpnn_init_fwd: input must not alias M0");
  const DmInitArgs a{num_nodes, num_edges, in_src, P, ldp, D, rows, De, (De + 3) / 4 * 4, W_ieT, b_i, input, ldi, M0, ldm};
  const hipStream_t st = as_stream(stream);
  const size_t wbytes = (size_t)De * D * 4;
  const bool lds = wbytes <= (size_t)kDmLdsBytes;
  const bool sub = D <= kDmSubD;
  const int64_t per_block = (256 / (sub ? 16 : 64)) * (lds ? kDmRows : 1);
  const unsigned grid = (unsigned)ceil_div(num_edges, per_block);
  if (sub && lds) dmpnn_init_kernel<16, true><<<grid, 256, wbytes, st>>>(a);
  else if (sub) dmpnn_init_kernel<16, false><<<grid, 256, 0, st>>>(a);
  else if (lds) dmpnn_init_kernel<64, true><<<grid, 256, wbytes, st>>>(a);
  else dmpnn_init_kernel<64, false><<<grid, 256, 0, st>>>(a);
  return check_launch("dmpnn_init_kernel");
}

extern "C" int mvml_dmpnn_update(int64_t num_nodes, int64_t num_edges, const int32_t* in_rowptr,
                                 const int32_t* out_rowptr, const int32_t* out_inslot, const int32_t* rev_slot,
                                 const float* R, int64_t ldr, const float* input, int64_t ldi, const float* b_h, int D,
                                 float* out, int64_t ldo, void* stream) {
  clear_error();
  MVML_REQUIRE(sizes_ok(num_nodes, num_edges), "dmpnn_update: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  MVML_REQUIRE(width_ok(D), "dmpnn_update: D must be a positive multiple of 4 <= %d (got %d)", kDmMaxD, D);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(num_nodes > 0 && in_rowptr != nullptr && out_rowptr != nullptr && out_inslot != nullptr && rev_slot != nullptr,
               "dmpnn_update: both row pointers, out_inslot and rev_slot are required");
  MVML_REQUIRE(row_ok(R, ldr, D) && row_ok(input, ldi, D) && row_ok(out, ldo, D) && aligned16(b_h),
               "dmpnn_update: R, input and out must be 16-byte aligned with row strides >= D that are multiples of 4, "
               "b_h 16-byte aligned or NULL");
  MVML_REQUIRE(apart(out, ldo, R, ldr, num_edges, D) && apart(out, ldo, input, ldi, num_edges, D),
               "dmpnn_update: out must not alias R or input");
  const DmUpdArgs a{num_nodes, in_rowptr, nullptr, out_rowptr, out_inslot, rev_slot, R, ldr, input, ldi, b_h, D, out, ldo,
                    nullptr, 0, nullptr, nullptr, 0};
  return launch_update<false>(a, as_stream(stream));
}

extern "C" int mvml_dmpnn_update_bwd(int64_t num_nodes, int64_t num_edges, const int32_t* in_rowptr,
                                     const int32_t* out_rowptr, const int32_t* out_inslot, const int32_t* rev_slot,
                                     const float* out, int64_t ldo, const float* g_out, int64_t ldg, int D, float* dR,
                                     int64_t lddr, float* dpre, int64_t lddp, void* stream) {
  clear_error();
  MVML_REQUIRE(sizes_ok(num_nodes, num_edges), "dmpnn_update_bwd: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  MVML_REQUIRE(width_ok(D), "dmpnn_update_bwd: D must be a positive multiple of 4 <= %d (got %d)", kDmMaxD, D);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(num_nodes > 0 && in_rowptr != nullptr && out_rowptr != nullptr && out_inslot != nullptr && rev_slot != nullptr,
               "dmpnn_update_bwd: both row pointers, out_inslot and rev_slot are required");
  MVML_REQUIRE(row_ok(out, ldo, D) && row_ok(g_out, ldg, D) && row_ok(dR, lddr, D) && row_ok(dpre, lddp, D),
               "dmpnn_update_bwd: out, g_out, dR and dpre must be 16-byte aligned with row strides >= D that are "
               "multiples of 4");
  MVML_REQUIRE(apart(dR, lddr, out, ldo, num_edges, D) && apart(dR, lddr, g_out, ldg, num_edges, D) &&
                   apart(dpre, lddp, out, ldo, num_edges, D) && apart(dpre, lddp, g_out, ldg, num_edges, D) &&
                   apart(dR, lddr, dpre, lddp, num_edges, D),
               "dmpnn_update_bwd: dR and dpre must not alias out, g_out or each other");
  const DmUpdArgs a{num_nodes, out_rowptr, out_inslot, in_rowptr, nullptr, rev_slot, g_out, ldg, out, ldo, nullptr, D, dR,
                    lddr, dpre, lddp, nullptr, nullptr, 0};
  return launch_update<true>(a, as_stream(stream));
}

extern "C" int mvml_dmpnn_atom_sum(int64_t num_nodes, int64_t num_edges, const int32_t* rowptr, const int32_t* idx,
                                   const float* M, int64_t ldm, int D, float* a_out, int64_t lda, void* stream) {
  clear_error();
  MVML_REQUIRE(sizes_ok(num_nodes, num_edges), "dmpnn_atom_sum: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  MVML_REQUIRE(width_ok(D), "dmpnn_atom_sum: D must be a positive multiple of 4 <= %d (got %d)", kDmMaxD, D);
  if (num_nodes == 0) return MVML_OK;
  MVML_REQUIRE(rowptr != nullptr && row_ok(a_out, lda, D) && (num_edges == 0 || row_ok(M, ldm, D)),
               "dmpnn_atom_sum: rowptr is required; M and a must be 16-byte aligned with row strides >= D that are "
               "multiples of 4");
  const DmUpdArgs a{num_nodes, rowptr, idx, nullptr, nullptr, nullptr, M, ldm, nullptr, 0, nullptr, D, nullptr, 0,
                    nullptr, 0, nullptr, a_out, lda};
  return launch_update<false>(a, as_stream(stream));
}

extern "C" int mvml_dmpnn_atom_sum_bwd(int64_t num_nodes, int64_t num_edges, const int32_t* in_rowptr, const float* g_a,
                                       int64_t ldg, int D, float* dM, int64_t lddm, void* stream) {
  clear_error();
  MVML_REQUIRE(sizes_ok(num_nodes, num_edges), "dmpnn_atom_sum_bwd: bad sizes %lld, %lld", (long long)num_nodes,
               (long long)num_edges);
  MVML_REQUIRE(width_ok(D), "dmpnn_atom_sum_bwd: D must be a positive multiple of 4 <= %d (got %d)", kDmMaxD, D);
  if (num_edges == 0) return MVML_OK;
  MVML_REQUIRE(num_nodes > 0 && in_rowptr != nullptr && row_ok(g_a, ldg, D) && row_ok(dM, lddm, D),
               "dmpnn_atom_sum_bwd: in_rowptr is required; g_a and dM must be 16-byte aligned with row strides >= D that "
               "are multiples of 4");
  const DmUpdArgs a{num_nodes, nullptr, nullptr, in_rowptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, D, dM, lddm,
                    nullptr, 0, g_a, nullptr, ldg};
  return launch_update<true>(a, as_stream(stream));
}
