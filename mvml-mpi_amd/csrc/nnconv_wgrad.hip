// NNConv's weight gradient on split-fp16 MFMA (the fp32 form is nnconv_wgrad_kernel, nnconv.hip):
//
//   dW2[(i, o), k] = sum_e (h[src e][i] dM[e][o]) z[e][k],  dM[e] = g_pre[slot_dst[e]]
//
// For one i this is C_i [D, H] = P_i^T [D, E] x Z [E, H] with P_i[e][o] = h[src e][i] dM[e][o], on
// v_mfma_f32_16x16x32_f16 with a chunk of kWgE = 32 edges as the instruction's k: lane (lr, lg) of
// an A fragment holds row o = 16 mt + lr at the edges 8 lg .. 8 lg + 7, of a B fragment column
// k = 16 nt + lr at the same edges.  Both are the transpose of how dM and z lie in memory.
//
// Scales.  A power-of-two scale may only be constant along the contracted axis, the edges here, so
// there are no per-row scales: three global maxima.  z is scaled by 2^sz (amax_shift of max |z|).
// p = h dM is formed in fp32 with one __fmul_rn and scaled by 2^(sh + sg - 15): |h| 2^sh and
// |dM| 2^sg are below 2^15 each, so |p| 2^(sh + sg) is below 2^30 and the - 15 brings it back
// under fp16's range.  Both are undone once, as the partials leave the kernel.  The split is
// split2h8's (h h + h l + l h, l l dropped).  max |h| and max |g_pre| are taken over the rows the
// edges reference (the entry point is not told the atom count), folded with the same unsigned
// atomicMax as absmax_launch.
//
// The z image (mvml_nnconv_split_z): z is the same for every message-passing step and every
// workgroup, so it is split and transposed once: chunk c, column block nt -> {h, l} x 64 lanes x
// 16 B in B-fragment order, the tail chunk zero-filled; a 256-byte header holds the bits of
// max |z|.  A B fragment in the hot loop is one coalesced 16-byte load per lane from L2: no LDS,
// no transpose, no split.
//
// nnconv_wgrad_f16x2_kernel: a workgroup of four waves owns IB consecutive values of i (grid x,
// fastest: concurrent workgroups share an edge range's z fragments in L2) and one edge range (grid
// y), and keeps ALL their accumulators in registers: a wave holds kWgTiles = 64 accumulator tiles
// (256 registers), so a chunk's B fragments and dM rows serve IB values of i instead of one.
//
// Wave split.  The four waves are a WM x WN x WI grid over (row blocks, column blocks, values of
// i), each factor the largest power of two that the extent fills:
//   WM = 4 if MT >= 4, 2 if MT >= 2, else 1;  WN = min(4 / WM, same rule on NT);  WI = 4 / (WM WN).
// Wave (wm, wn, wi) owns the row blocks mt = wm (mod WM), the column blocks nt = wn (mod WN) and
// the i values ii = wi (mod WI) of the workgroup's IB.  So with MT >= 4 every wave prepares the A
// fragments of its own row blocks only (none is prepared twice), and at D = 16 or H = 16 the
// waves that have no block of their own on that axis take other columns or other values of i
// instead of idling.  The kernel is instantiated on (MW, NW, IW), the per-wave extents rounded up
// (MW <= 2, NW a power of two <= 16, IW = min(16, 64 / (MW NW))); IB = min(IW WI, D).  That is
// IB = 8 at (64, 128) and 2 at (128, 256).
//
// dM goes through LDS once per chunk: the 32 gathered rows as fp32 at a row pitch of D + 2 floats.
// A lane reads column 16 mt + lr of the rows 8 lg + j, one j at a time: the 16 lr are consecutive
// banks and the four lg must land 16 banks apart, so 8 pitch = 16 (mod 64), pitch = 2 (mod 8)
// (which also holds with 32 banks and half a wave per pass).  nn_pitch's pitch = 16 (mod 64)
// would put all four lg on the same banks.  Rows are therefore stored with 8-byte stores.
// h[src e][i0 .. i0 + IB) is staged transposed beside it ([ii][32]: a lane's eight edges are two
// 16-byte reads).  A wave keeps its dM fragments as fp32 in registers across its i loop; per i:
// eight multiplies by the edge's h, one split2h8, then 3 x (its column blocks) MFMAs.
//
// Pipeline: the next chunk's global loads (dM rows, h columns, the first B fragments; the row
// indices come a chunk earlier still) are issued before the current chunk's MFMAs and parked in
// the other LDS buffer after them: two buffers, one barrier per chunk.
//
// Edge ranges: S ranges of whole chunks so that (D / IB) x S workgroups fill the device; the
// per-range partials are summed in fixed order by colsum_final_launch (beta = 1 when
// accumulating).  No float atomics: two runs agree bitwise.
#include "gemm_common.h"

namespace mvml {
namespace {

constexpr int kWgE = 32;         // edges per chunk: one k-step of v_mfma_f32_16x16x32_f16
constexpr int kWgTiles = 64;     // accumulator tiles per wave (x 4 registers)
constexpr int kWgMaxRanges = 64;
constexpr int kWgGroups = 256;   // workgroups wanted in flight: one per CU
constexpr int kNnTile = 128;     // (nnconv.hip's edge tile: the same bound on E)

__device__ __forceinline__ float4 wg_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

struct WgPlan {
  int WM, WN, WI;  // the wave grid
  int MW, NW, IW;  // the kernel instance: per-wave extents
  int IB;          // values of i per workgroup
};
inline int wg_pow2_le4(int x) { return x >= 4 ? 4 : x >= 2 ? 2 : 1; }
WgPlan wg_plan(int D, int H) {
  const int MT = D / 16, NT = H / 16;
  WgPlan p;
  p.WM = wg_pow2_le4(MT);
  p.WN = std::min(4 / p.WM, wg_pow2_le4(NT));
  p.WI = 4 / (p.WM * p.WN);
  p.MW = (int)ceil_div(MT, p.WM);
  const int nw = (int)ceil_div(NT, p.WN);
  p.NW = 1;
  while (p.NW < nw) p.NW *= 2;
  p.IW = std::min(16, kWgTiles / (p.MW * p.NW));
  p.IB = std::min(p.IW * p.WI, D);
  return p;
}

// The edge ranges: S of them, `per` whole chunks each, none empty.
struct WgRanges {
  int S;
  int64_t per;
};
WgRanges wg_ranges(int64_t E, int D, int H) {
  const int64_t chunks = std::max<int64_t>(1, ceil_div(E, kWgE));
  const int64_t blocks = ceil_div(D, wg_plan(D, H).IB);
  const int64_t want = std::min<int64_t>(std::min<int64_t>(ceil_div(kWgGroups, blocks), kWgMaxRanges), chunks);
  WgRanges r;
  r.per = ceil_div(chunks, want);
  r.S = (int)ceil_div(chunks, r.per);
  return r;
}

size_t z_image_vec(int64_t E, int H) { return (size_t)ceil_div(E, kWgE) * (H / 16) * 128; }

// The z image: one thread per (chunk, column block, lane), eight edges each.
__global__ void __launch_bounds__(256)
nnconv_split_z_kernel(int64_t E, int H, const float* __restrict__ z, int64_t ldz, const uint32_t* __restrict__ amax,
                      uint4* __restrict__ img) {
  const int NT = H / 16;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ceil_div(E, kWgE) * NT * 64) return;
  const int lane = (int)(idx & 63), lr = lane & 15, lg = lane >> 4;
  const int nt = (int)((idx >> 6) % NT);
  const int64_t c = (idx >> 6) / NT;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t e = c * kWgE + 8 * lg + j;
    v[j] = e < E ? z[e * ldz + 16 * nt + lr] : 0.f;
  }
  bf16x8 h, l;
  split2h8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), pow2f(amax_shift(*amax)), h, l);
  uint4* dst = img + (c * NT + nt) * 128 + lane;
  dst[0] = __builtin_bit_cast(uint4, h);
  dst[64] = __builtin_bit_cast(uint4, l);
}

__global__ void nnconv_wgrad_clear_kernel(uint32_t* out) {
  if (threadIdx.x < 2) out[threadIdx.x] = 0u;
}

// out[0], out[1] = bits of max |h[src e]|, max |g[slot_dst e]| over the edges: a thread per float4,
// grid-stride, one atomicMax pair per workgroup (unsigned, order-independent).
__global__ void __launch_bounds__(256)
nnconv_wgrad_amax_kernel(int64_t E, int D, const int32_t* __restrict__ slot_dst, const int32_t* __restrict__ src,
                         const float* __restrict__ h, int64_t ldh, const float* __restrict__ g, int64_t ldg,
                         uint32_t* __restrict__ out) {
  const int QD = D / 4;
  float mh = 0.f, mg = 0.f;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < E * QD; t += (int64_t)gridDim.x * 256) {
    const int64_t e = t / QD;
    const int c = 4 * (int)(t - e * QD);
    const float4 a = wg_ld4(h + (int64_t)src[e] * ldh + c), b = wg_ld4(g + (int64_t)slot_dst[e] * ldg + c);
    mh = fmaxf(mh, fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))));
    mg = fmaxf(mg, fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
  }
  mh = wave_max(mh);
  mg = wave_max(mg);
  __shared__ float red[2][4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mh;
    red[1][threadIdx.x >> 6] = mg;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const float* r = red[threadIdx.x];
    atomicMax(out + threadIdx.x, __float_as_uint(fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]))));
  }
}

struct WgArgs {
  int64_t E;
  int64_t per;              // chunks per edge range
  const int32_t* slot_dst;
  const int32_t* src;
  const float* h;
  int64_t ldh;
  const float* g;
  int64_t ldg;
  int D, H;
  const uint4* img;         // the z image's fragments
  const uint32_t* amax_z;   // its header: bits of max |z|
  const uint32_t* amax_hg;  // bits of max |h|, max |g|
  float* part;              // [ranges][D * D * H]
  int WM, WN, WI, IB;
};

template <int MW, int NW, int IW>
__global__ void __launch_bounds__(256) nnconv_wgrad_f16x2_kernel(WgArgs a) {
  constexpr int PF = NW <= 8 ? NW : 2;  // B fragments fetched a chunk ahead
  constexpr int kStage = 4;             // float4 of dM / values of h per thread and chunk (D <= 128, IB <= 32)
  extern __shared__ float sm[];
  const int D = a.D, H = a.H, MT = D / 16, NT = H / 16, QD = D / 4, PD = D + 2, IB = a.IB;
  float* gs = sm;                   // [2][32][PD] dM rows
  float* hT = sm + 2 * kWgE * PD;   // [2][IB][32] h[src e][i0 + ii]
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % a.WM, wn = (wave / a.WM) % a.WN, wi = wave / (a.WM * a.WN);
  const int i0 = blockIdx.x * IB;
  const int64_t cb = (int64_t)blockIdx.y * a.per, ce = min(ceil_div(a.E, (int64_t)kWgE), cb + a.per);

  // what this thread stages per chunk: dM float4 (row gr, column gc) and h value (edge tid % 32, ii = hi)
  int gr[kStage], gc[kStage];
#pragma unroll
  for (int l = 0; l < kStage; ++l) {
    const int idx = tid + 256 * l;
    gr[l] = idx < kWgE * QD ? idx / QD : -1;
    gc[l] = 4 * (idx % QD);
  }
  const int he = tid & 31, hi = tid >> 5;
  int nid[kStage], nsrc;   // row indices of the chunk whose rows are loaded next (-1: zeros)
  float4 gq[kStage];
  float hq[kStage];
  auto load_idx = [&](int64_t c) {
#pragma unroll
    for (int l = 0; l < kStage; ++l) {
      const int64_t s = c * kWgE + gr[l];
      nid[l] = (gr[l] >= 0 && c < ce && s < a.E) ? a.slot_dst[s] : -1;
    }
    const int64_t s = c * kWgE + he;
    nsrc = (c < ce && s < a.E) ? a.src[s] : -1;
  };
  auto load_rows = [&]() {
#pragma unroll
    for (int l = 0; l < kStage; ++l)
      gq[l] = nid[l] >= 0 ? wg_ld4(a.g + (int64_t)nid[l] * a.ldg + gc[l]) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int l = 0; l < kStage; ++l) {
      const int ii = hi + 8 * l;
      hq[l] = (nsrc >= 0 && ii < IB && i0 + ii < D) ? a.h[(int64_t)nsrc * a.ldh + i0 + ii] : 0.f;
    }
  };
  auto park = [&](int buf) {
#pragma unroll
    for (int l = 0; l < kStage; ++l)
      if (gr[l] >= 0) {
        float* p = gs + (buf * kWgE + gr[l]) * PD + gc[l];  // (PD = 2 mod 8: 8-byte aligned, not 16)
        *reinterpret_cast<float2*>(p) = make_float2(gq[l].x, gq[l].y);
        *reinterpret_cast<float2*>(p + 2) = make_float2(gq[l].z, gq[l].w);
      }
#pragma unroll
    for (int l = 0; l < kStage; ++l) {
      const int ii = hi + 8 * l;
      if (ii < IB) hT[(buf * IB + ii) * kWgE + he] = hq[l];
    }
  };
  // B fragments: bh / bl of the current chunk, nh / nl the first PF of the next
  u32x4 bh[NW] = {}, bl[NW] = {}, nh[PF] = {}, nl[PF] = {};
  auto frag = [&](int64_t c, int j) { return a.img + (c * NT + wn + a.WN * j) * 128 + lane; };
  auto fetch_next = [&](int64_t c) {
#pragma unroll
    for (int j = 0; j < PF; ++j)
      if (wn + a.WN * j < NT) {
        nh[j] = __builtin_bit_cast(u32x4, frag(c, j)[0]);
        nl[j] = __builtin_bit_cast(u32x4, frag(c, j)[64]);
      }
  };

  const int sp = min(120, max(-120, amax_shift(a.amax_hg[0]) + amax_shift(a.amax_hg[1]) - 15));
  const float ps = pow2f(sp);
  f32x4 acc[IW][MW][NW];
#pragma unroll
  for (int q = 0; q < IW; ++q)
#pragma unroll
    for (int m = 0; m < MW; ++m)
#pragma unroll
      for (int j = 0; j < NW; ++j) acc[q][m][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (cb < ce) {
    load_idx(cb);
    load_rows();
    fetch_next(cb);
    load_idx(cb + 1);
    park(0);
  }
  __syncthreads();
  int buf = 0;
  for (int64_t c = cb; c < ce; ++c, buf ^= 1) {
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      if (j < PF) {
        bh[j] = nh[j];
        bl[j] = nl[j];
      } else if (wn + a.WN * j < NT) {
        bh[j] = __builtin_bit_cast(u32x4, frag(c, j)[0]);
        bl[j] = __builtin_bit_cast(u32x4, frag(c, j)[64]);
      }
    }
    const bool more = c + 1 < ce;  // (uniform over the workgroup)
    if (more) {
      load_rows();
      fetch_next(c + 1);
      load_idx(c + 2);
    }
    // the wave's dM fragments, fp32: row block m, column 16 mt + lr, edges 8 lg + j
    float dm[MW][8];
#pragma unroll
    for (int m = 0; m < MW; ++m)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dm[m][j] = wm + a.WM * m < MT ? gs[(buf * kWgE + 8 * lg + j) * PD + 16 * (wm + a.WM * m) + lr] : 0.f;
#pragma unroll
    for (int q = 0; q < IW; ++q) {
      const int ii = wi + a.WI * q;
      if (ii >= IB || i0 + ii >= D) continue;  // (uniform over the wave)
      const float4 h0 = wg_ld4(hT + (buf * IB + ii) * kWgE + 8 * lg), h1 = wg_ld4(hT + (buf * IB + ii) * kWgE + 8 * lg + 4);
      f16x8 ah[MW], al[MW];
#pragma unroll
      for (int m = 0; m < MW; ++m) {
        const float4 p0 = make_float4(__fmul_rn(h0.x, dm[m][0]), __fmul_rn(h0.y, dm[m][1]), __fmul_rn(h0.z, dm[m][2]),
                                      __fmul_rn(h0.w, dm[m][3]));
        const float4 p1 = make_float4(__fmul_rn(h1.x, dm[m][4]), __fmul_rn(h1.y, dm[m][5]), __fmul_rn(h1.z, dm[m][6]),
                                      __fmul_rn(h1.w, dm[m][7]));
        bf16x8 hh, ll;
        split2h8(p0, p1, ps, hh, ll);
        ah[m] = __builtin_bit_cast(f16x8, hh);
        al[m] = __builtin_bit_cast(f16x8, ll);
      }
      // the three products, each over all the wave's tiles of this i: dependent MFMAs stay apart
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int m = 0; m < MW; ++m) {
          if (wm + a.WM * m >= MT) continue;
#pragma unroll
          for (int j = 0; j < NW; ++j) {
            if (wn + a.WN * j >= NT) continue;
            const f16x8 av = t == 0 ? al[m] : ah[m];
            const f16x8 bv = __builtin_bit_cast(f16x8, t == 1 ? bl[j] : bh[j]);
            acc[q][m][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc[q][m][j], 0, 0, 0);
          }
        }
    }
    if (more) park(buf ^ 1);
    __syncthreads();
  }

  // the accumulators' layout: rows o = 16 mt + 4 lg + r, column k = 16 nt + lr
  const float up = pow2f(-sp), uz = pow2f(-amax_shift(*a.amax_z));
  float* pp = a.part + (int64_t)blockIdx.y * D * D * H;
#pragma unroll
  for (int q = 0; q < IW; ++q) {
    const int ii = wi + a.WI * q;
    if (ii >= IB || i0 + ii >= D) continue;
#pragma unroll
    for (int m = 0; m < MW; ++m) {
      const int mt = wm + a.WM * m;
      if (mt >= MT) continue;
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        const int nt = wn + a.WN * j;
        if (nt >= NT) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pp[((int64_t)(i0 + ii) * D + 16 * mt + 4 * lg + r) * H + 16 * nt + lr] = acc[q][m][j][r] * up * uz;
      }
    }
  }
}

int check_nnconv(const char* who, int D, int H) {
  MVML_REQUIRE(D >= 16 && D <= 128 && D % 16 == 0, "%s: node width must be a multiple of 16 in [16, 128] (got %d)", who, D);
  MVML_REQUIRE(H >= 16 && H <= 256 && H % 16 == 0, "%s: edge hidden width must be a multiple of 16 in [16, 256] (got %d)", who, H);
  return MVML_OK;
}
bool edges_ok(int64_t E) { return E >= 0 && E < (int64_t(1) << 31) - kNnTile; }

int launch_wgrad(const WgArgs& a, const WgPlan& p, int S, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.D, p.IB), (unsigned)S);
  const size_t lds = (size_t)(2 * kWgE * (a.D + 2) + 2 * p.IB * kWgE) * 4;
  auto go = [&](auto mw, auto nw) {
    constexpr int MW = decltype(mw)::value, NW = decltype(nw)::value;
    constexpr int IW = kWgTiles / (MW * NW) < 16 ? kWgTiles / (MW * NW) : 16;
    nnconv_wgrad_f16x2_kernel<MW, NW, IW><<<grid, 256, lds, st>>>(a);
    return MVML_OK;
  };
  switch_const<1, 2>(p.MW, [&](auto mw) { return switch_const<1, 2, 4, 8, 16>(p.NW, [&](auto nw) { return go(mw, nw); }); });
  return check_launch("nnconv_wgrad_f16x2_kernel");
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" size_t mvml_nnconv_z_image_bytes(int64_t num_edges, int H) {
  if (!edges_ok(num_edges) || H < 16 || H > 256 || H % 16) return 0;
  return 256 + 16 * z_image_vec(num_edges, H);
}

extern "C" int mvml_nnconv_split_z(int64_t num_edges, int H, const float* z, int64_t ldz, void* image, void* stream) {
  clear_error();
  MVML_REQUIRE(H >= 16 && H <= 256 && H % 16 == 0, "nnconv_split_z: edge hidden width must be a multiple of 16 in [16, 256] (got %d)", H);
  MVML_REQUIRE(edges_ok(num_edges), "nnconv_split_z: bad num_edges %lld", (long long)num_edges);
  MVML_REQUIRE(image != nullptr && aligned16(image), "nnconv_split_z: a 16-byte aligned image is required");
  MVML_REQUIRE(num_edges == 0 || row_ok(z, ldz, H),
               "nnconv_split_z: with edges, z must be 16-byte aligned with a pitch >= H that is a multiple of 4");
  const hipStream_t st = as_stream(stream);
  uint32_t* amax = static_cast<uint32_t*>(image);
  if (int rc = absmax_launch(num_edges, H, z, ldz, amax, false, st)) return rc;
  if (num_edges == 0) return MVML_OK;
  const int64_t n = (int64_t)z_image_vec(num_edges, H) / 2;
  nnconv_split_z_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(
      num_edges, H, z, ldz, amax, reinterpret_cast<uint4*>(static_cast<char*>(image) + 256));
  return check_launch("nnconv_split_z_kernel");
}

extern "C" size_t mvml_nnconv_bwd_weight_f16x2_workspace_size(int64_t num_edges, int D, int H) {
  if (!edges_ok(num_edges) || D < 16 || D > 128 || D % 16 || H < 16 || H > 256 || H % 16) return 0;
  // the ranges' partials, then the two maxima
  return carve_size((size_t)wg_ranges(num_edges, D, H).S * D * D * H * 4) + carve_size(2 * sizeof(uint32_t)) + 256;
}

extern "C" int mvml_nnconv_bwd_weight_f16x2(int64_t num_edges, const int32_t* in_src, const int32_t* slot_dst,
                                            const float* h, int64_t ldh, int D, const float* z, int64_t ldz, int H,
                                            const float* g_out, int64_t ldg, int accumulate, float* dW2,
                                            void* workspace, size_t workspace_bytes, void* stream,
                                            const void* z_image) {
  clear_error();
  if (int rc = check_nnconv("nnconv_bwd_weight_f16x2", D, H)) return rc;
  MVML_REQUIRE(edges_ok(num_edges), "nnconv_bwd_weight_f16x2: bad num_edges %lld", (long long)num_edges);
  MVML_REQUIRE(dW2 != nullptr && aligned16(dW2), "nnconv_bwd_weight_f16x2: a 16-byte aligned dW2 is required");
  const int64_t n = (int64_t)D * D * H;
  if (num_edges == 0) return accumulate ? MVML_OK : mvml_fill_zero(dW2, 1, n * 4, n * 4, stream);
  MVML_REQUIRE(row_ok(h, ldh, D) && row_ok(g_out, ldg, D) && row_ok(z, ldz, H) && in_src != nullptr && slot_dst != nullptr,
               "nnconv_bwd_weight_f16x2: h, g_out (pitches >= D) and z (pitch >= H) must be 16-byte aligned with pitches "
               "that are multiples of 4; in_src and slot_dst are required");
  MVML_REQUIRE(z_image != nullptr && aligned16(z_image),
               "nnconv_bwd_weight_f16x2: with edges, the 16-byte aligned z image (mvml_nnconv_split_z) is required");
  const size_t need = mvml_nnconv_bwd_weight_f16x2_workspace_size(num_edges, D, H);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("nnconv_bwd_weight_f16x2: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVML_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  const WgPlan p = wg_plan(D, H);
  const WgRanges rg = wg_ranges(num_edges, D, H);
  Carver cv(workspace, workspace_bytes);
  float* part = cv.take<float>((size_t)rg.S * n);
  uint32_t* amax_hg = cv.take<uint32_t>(2);
  nnconv_wgrad_clear_kernel<<<1, 64, 0, st>>>(amax_hg);
  if (int rc = check_launch("nnconv_wgrad_clear_kernel")) return rc;
  const unsigned ab = (unsigned)std::min<int64_t>(ceil_div(num_edges * (D / 4), 256), 1024);
  nnconv_wgrad_amax_kernel<<<ab, 256, 0, st>>>(num_edges, D, slot_dst, in_src, h, ldh, g_out, ldg, amax_hg);
  if (int rc = check_launch("nnconv_wgrad_amax_kernel")) return rc;
  WgArgs a{};
  a.E = num_edges; a.per = rg.per; a.slot_dst = slot_dst; a.src = in_src; a.h = h; a.ldh = ldh; a.g = g_out; a.ldg = ldg;
  a.D = D; a.H = H; a.img = reinterpret_cast<const uint4*>(static_cast<const char*>(z_image) + 256);
  a.amax_z = static_cast<const uint32_t*>(z_image); a.amax_hg = amax_hg; a.part = part;
  a.WM = p.WM; a.WN = p.WN; a.WI = p.WI; a.IB = p.IB;
  if (int rc = launch_wgrad(a, p, rg.S, st)) return rc;
  return colsum_final_launch(n, rg.S, part, n, 1.f, accumulate ? 1.f : 0.f, dW2, st, "nnconv_bwd_weight_f16x2 (partial sum)");
}
