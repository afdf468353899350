// Small-K split-fp16 product: the layer-1 projection as the memory kernel it is (behind
// mvml_gemm_f16x2_rows, gemm_f32.hip).
//
// C[M][N] = A[M][K] B[N][K]^T for K <= 96 (the atom features: K = 76 against the 1544 rows of
// layer 1's Wcat) writes N / K ~ 20 output bytes per input byte: HBM-bound on the C stores, and
// the 256x256 tile (five 16-deep stages, then an LDS epilogue that cannot overlap the next
// tile's loads) reached 0.34 of HBM on it.  Here a WAVE owns 64 output columns: it loads the
// split-fp16 planes of its 64 B rows into registers ONCE (B's il4 image, or fp32 split in place
// -- bitwise the same planes), then walks chunk_blocks blocks of 16 A rows: A's fragments come
// straight from global memory (the next block's in flight behind the current block's MFMAs),
// are split with the row's own scale (split2h, as the tiles do) and multiplied as C^T = B A^T
// on v_mfma_f32_16x16x32_f16 (K <= 16: 16x16x16) — transposed so that each lane's four
// accumulators are FOUR CONSECUTIVE COLUMNS OF ONE ROW; a wave-private LDS slice turns the
// 16 x 64 block into 4-row x 256-B float4 stores (measured: float4 stores straight from the
// accumulators, 16 rows x 64 B per instruction, ran at the tile's 2.7 TB/s), no block barrier.  The
// three products per k-step keep the tiles' order (l_b h_a, h_b l_a, h_b h_a); the scales are
// undone as there (B's, then the row's).  Waves are numbered XCD-major (xcd_block), slab
// fastest: the ~25 waves sharing a block of A rows run together on one XCD and read the rows
// from its L2.  Same values as the tiles to fp32-GEMM accuracy (the MFMA shape changes the
// summation order, so not bitwise).
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "gemm_common.h"

namespace mvml {
namespace {

constexpr int kSkMaxK = 96;

// KS16 = ceil(K / 16): KS16 / 2 steps of 16x16x32 and, for odd KS16, a 16-deep tail on
// 16x16x16, each zero-padded past K.  The tail accumulates into its OWN registers, added once at
// the end: behind 16x16x32 steps on the same accumulators it came out wrong in the first two of
// each lane's four results (K = 76 / 80, a missing MFMA-to-MFMA wait between the two pass
// counts).  Skipping the 16 padding k of a 96-deep plan saves 1/6 of the MFMA time at K = 76.
// A rows with an all-zero low plane (fp16-exact values: layer 1's 0/1 atom features) skip the
// h_b l_a products — per 16-row block, wave-uniform (a ballot); adding exact zeros is all they
// would do.
// ABL (timing ablations, option smallk 5 / 6; wrong results): 1 = no MFMAs, 2 = no C stores
// WL (default): the workgroup's four waves share ONE 64-column slab (four consecutive row
// chunks) and its B planes live in LDS (filled once, one group per wave), read per block as
// fragments — no B registers (162 VGPRs instead of 230), so three waves fit per SIMD and the
// store stream overlaps more matrix work: 3.26 -> 2.75 ms at config 3 on one box.  WL = false
// (B fragments in registers, every wave its own slab) stays as option smallk 10.
template <int KS16, bool IL4, bool NT, int ABL = 0, int NG = 4, bool WL = false>
__global__ void __launch_bounds__(256, WL ? 3 : 2)  // two (three) waves per SIMD
gemm_smallk_kernel(int64_t M, int64_t N, int K, const float* __restrict__ A, int64_t lda,
                   const float* __restrict__ B, int64_t ldb, const uint32_t* __restrict__ a_rows,
                   const uint32_t* __restrict__ amax_b, const float* __restrict__ bias, int act,
                   float* __restrict__ C, int64_t ldc, int n_slabs, int chunk_blocks) {
  constexpr int N32 = KS16 / 2, T16 = KS16 % 2, NW = N32 > 0 ? N32 : 1;
  constexpr int NX = 2 * N32 + T16;  // A float4 per lane and row block
  constexpr int SW = 16 * NG, PITCH = SW + 4;  // slab width (columns per wave); LDS row pitch
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t lb = xcd_block(blockIdx.x, gridDim.x);
  const int64_t w = lb * 4 + wid;
  const int slab = (int)(WL ? lb % n_slabs : w % n_slabs);
  const int64_t nrb = (M + 15) >> 4;
  const int64_t rb0 = (WL ? (lb / n_slabs) * 4 + wid : w / n_slabs) * chunk_blocks;
  if (!WL && rb0 >= nrb) return;
  const int64_t rb1 = min(nrb, rb0 + (int64_t)chunk_blocks);
  const int kb = amax_shift(*amax_b);
  const float s_b = pow2f(kb), u_b = pow2f(-kb);
  // this lane's B rows (output columns c0 + 16 g + li) for the MFMA's A side: k = 32 s + 8 lq
  // + 0..7 (x32 steps), 32 N32 + 4 lq + 0..3 (x16 tail); k >= K reads as zero
  constexpr int RG = WL ? 1 : NG;  // register copies of the B fragments (WL: none)
  f16x8 bh[RG][NW], bl[RG][NW];
  f16x4 th[RG], tl[RG];
  __shared__ u32x4 s_wh[WL ? NG : 1][WL ? NW : 1][WL ? 64 : 1], s_wl[WL ? NG : 1][WL ? NW : 1][WL ? 64 : 1];
  __shared__ uint2 s_th[WL ? NG : 1][WL ? 64 : 1], s_tl[WL ? NG : 1][WL ? 64 : 1];
  auto piece = [&](const float* row, int k, uint2& h, uint2& l) {  // B[row][k .. k + 3] as planes
    const float4 v = *reinterpret_cast<const float4*>(row + min(k, K - 4));
    if constexpr (IL4) {
      h = make_uint2(__float_as_uint(v.x), __float_as_uint(v.y));
      l = make_uint2(__float_as_uint(v.z), __float_as_uint(v.w));
    } else {
      split2h(v, s_b, h, l);
    }
    if (k >= K) h = l = make_uint2(0u, 0u);
  };
  if constexpr (WL) {  // wave wid fills group wid's planes (NG == 4 waves), then one barrier
    static_assert(NG == 4, "one group per wave");
    const int g = wid;
    const int64_t col = (int64_t)slab * SW + 16 * g + li;
    const float* row = B + min(col, N - 1) * ldb;
#pragma unroll
    for (int s = 0; s < N32; ++s) {
      uint2 h0, l0, h1, l1;
      piece(row, 32 * s + 8 * lq, h0, l0);
      piece(row, 32 * s + 8 * lq + 4, h1, l1);
      s_wh[g][s][lane] = u32x4{h0.x, h0.y, h1.x, h1.y};
      s_wl[g][s][lane] = u32x4{l0.x, l0.y, l1.x, l1.y};
    }
    if constexpr (T16) {
      uint2 h, l;
      piece(row, 32 * N32 + 4 * lq, h, l);
      s_th[g][lane] = h;
      s_tl[g][lane] = l;
    }
    __syncthreads();
    if (rb0 >= nrb) return;
  } else {
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t col = (int64_t)slab * SW + 16 * g + li;
    const float* row = B + min(col, N - 1) * ldb;
#pragma unroll
    for (int s = 0; s < N32; ++s) {
      uint2 h0, l0, h1, l1;
      piece(row, 32 * s + 8 * lq, h0, l0);
      piece(row, 32 * s + 8 * lq + 4, h1, l1);
      const u32x4 hv = {h0.x, h0.y, h1.x, h1.y}, lv = {l0.x, l0.y, l1.x, l1.y};
      bh[g][s] = __builtin_bit_cast(f16x8, hv);
      bl[g][s] = __builtin_bit_cast(f16x8, lv);
    }
    if constexpr (T16) {
      uint2 h, l;
      piece(row, 32 * N32 + 4 * lq, h, l);
      th[g] = __builtin_bit_cast(f16x4, h);
      tl[g] = __builtin_bit_cast(f16x4, l);
    }
  }
  }
  // the B fragments of group g (registers, or the LDS image)
  auto fbh = [&](int g, int s) -> f16x8 {
    if constexpr (WL) return __builtin_bit_cast(f16x8, s_wh[g][s][lane]); else return bh[g][s];
  };
  auto fbl = [&](int g, int s) -> f16x8 {
    if constexpr (WL) return __builtin_bit_cast(f16x8, s_wl[g][s][lane]); else return bl[g][s];
  };
  auto fth = [&](int g) -> f16x4 {
    if constexpr (WL) return __builtin_bit_cast(f16x4, s_th[g][lane]); else return th[g];
  };
  auto ftl = [&](int g) -> f16x4 {
    if constexpr (WL) return __builtin_bit_cast(f16x4, s_tl[g][lane]); else return tl[g];
  };
  float bv[NG][4];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t col = (int64_t)slab * SW + 16 * g + 4 * lq + u;
      bv[g][u] = (bias && col < N) ? bias[col] : 0.f;
    }
  // A fragments of one 16-row block: row 16 rb + li, k as B's; KS16 float4 per lane
  auto load_a = [&](int64_t rb, float4 (&x)[NX], uint32_t& rbits) {
    const int64_t r = min(rb * 16 + li, M - 1);
    const float* p = A + r * lda;
#pragma unroll
    for (int s = 0; s < N32; ++s) {
      x[2 * s] = *reinterpret_cast<const float4*>(p + min(32 * s + 8 * lq, K - 4));
      x[2 * s + 1] = *reinterpret_cast<const float4*>(p + min(32 * s + 8 * lq + 4, K - 4));
    }
    if constexpr (T16) x[NX - 1] = *reinterpret_cast<const float4*>(p + min(32 * N32 + 4 * lq, K - 4));
    rbits = a_rows[r];
  };
  __shared__ __attribute__((aligned(16))) float s_c[4][16 * PITCH];
  float* wl = s_c[threadIdx.x >> 6];
  // two register sets, prefetch distance 2: a block's A rows are requested two blocks before
  // they are split (the first of the ~25 waves reading a row block pays the HBM miss)
  auto block = [&](int64_t rb, float4 (&xn)[NX], uint32_t& rn) {
    float4 x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = xn[i];
    const int ka = amax_shift(rn);
    if (rb + 2 < rb1) load_a(rb + 2, xn, rn);
    const float s_a = pow2f(ka);
    f16x8 ah[NW], al[NW];
    f16x4 ath, atl;
#pragma unroll
    for (int s = 0; s < N32; ++s) {
      uint2 h0, l0, h1, l1;
      split2h(x[2 * s], s_a, h0, l0);
      split2h(x[2 * s + 1], s_a, h1, l1);
      if (32 * s + 8 * lq >= K) h0 = l0 = make_uint2(0u, 0u);
      if (32 * s + 8 * lq + 4 >= K) h1 = l1 = make_uint2(0u, 0u);
      const u32x4 hv = {h0.x, h0.y, h1.x, h1.y}, lv = {l0.x, l0.y, l1.x, l1.y};
      ah[s] = __builtin_bit_cast(f16x8, hv);
      al[s] = __builtin_bit_cast(f16x8, lv);
    }
    if constexpr (T16) {
      uint2 h, l;
      split2h(x[NX - 1], s_a, h, l);
      if (32 * N32 + 4 * lq >= K) h = l = make_uint2(0u, 0u);
      ath = __builtin_bit_cast(f16x4, h);
      atl = __builtin_bit_cast(f16x4, l);
    }
    // any non-zero word in the block's A low plane (wave-uniform)
    uint32_t lo_bits = 0;
#pragma unroll
    for (int s = 0; s < N32; ++s) {
      const u32x4 q = __builtin_bit_cast(u32x4, al[s]);
      lo_bits |= q[0] | q[1] | q[2] | q[3];
    }
    if constexpr (T16) {
      const uint2 q = __builtin_bit_cast(uint2, atl);
      lo_bits |= q.x | q.y;
    }
    const bool a_lo = __ballot(lo_bits != 0) != 0;
    f32x4 acc[NG];
    auto products = [&](auto ALO) {
      constexpr bool kLo = decltype(ALO)::value;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (ABL == 1) {
#pragma unroll
          for (int s = 0; s < N32; ++s) {
            acc[g][0] += (float)ah[s][g] * (float)fbh(g, s)[0];
            acc[g][1] += (float)al[s][g] * (float)fbl(g, s)[1];
          }
          continue;
        }
#pragma unroll
        for (int s = 0; s < N32; ++s) {
          const f16x8 bhv = fbh(g, s), blv = fbl(g, s);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(blv, ah[s], acc[g], 0, 0, 0);
          if constexpr (kLo) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bhv, al[s], acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bhv, ah[s], acc[g], 0, 0, 0);
        }
      }
      if constexpr (T16 && ABL != 1) {
        f32x4 tac[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          tac[g] = f32x4{0.f, 0.f, 0.f, 0.f};
          const f16x4 thv = fth(g), tlv = ftl(g);
          tac[g] = __builtin_amdgcn_mfma_f32_16x16x16f16(tlv, ath, tac[g], 0, 0, 0);
          if constexpr (kLo) tac[g] = __builtin_amdgcn_mfma_f32_16x16x16f16(thv, atl, tac[g], 0, 0, 0);
          tac[g] = __builtin_amdgcn_mfma_f32_16x16x16f16(thv, ath, tac[g], 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = N32 > 0 ? acc[g] + tac[g] : tac[g];
      }
    };
    if (a_lo)
      products(std::true_type{});
    else
      products(std::false_type{});
    // the 16 x 64 block leaves through the wave's LDS slice: each lane's 4 x float4 (row li,
    // columns 16 g + 4 lq) in, then 4 rows x 256 contiguous bytes per store instruction out
    // (straight from the accumulators a store instruction would write 16 rows x 64 B)
    const float u_a = pow2f(-ka);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      float4 o;
      o.x = acc[g][0] * u_b * u_a + bv[g][0];
      o.y = acc[g][1] * u_b * u_a + bv[g][1];
      o.z = acc[g][2] * u_b * u_a + bv[g][2];
      o.w = acc[g][3] * u_b * u_a + bv[g][3];
      if (act == 1) {
        o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
      }
      *reinterpret_cast<float4*>(wl + li * PITCH + 16 * g + 4 * lq) = o;
    }
    wave_sync_lds();
#pragma unroll
    for (int t = 0; t < NG; ++t) {  // 64 / (4 NG) rows of SW floats per store instruction
      const int rr = (16 / NG) * t + lane / (4 * NG), c4 = 4 * (lane % (4 * NG));
      const float4 o = *reinterpret_cast<const float4*>(wl + rr * PITCH + c4);
      const int64_t row = rb * 16 + rr, col = (int64_t)slab * SW + c4;
      if (row < M && col < N && (ABL != 2 || __float_as_uint(o.x) == 0x7fc00123u)) {
        if constexpr (NT) {
          const f32x4 ov = {o.x, o.y, o.z, o.w};
          __builtin_nontemporal_store(ov, reinterpret_cast<f32x4*>(C + row * ldc + col));
        } else {
          *reinterpret_cast<float4*>(C + row * ldc + col) = o;
        }
      }
    }
    wave_sync_lds();  // the reads are done before the next block's writes
  };
  float4 xa[NX], xb[NX];
  uint32_t ra = 0, rbits = 0;
  load_a(rb0, xa, ra);
  if (rb0 + 1 < rb1) load_a(rb0 + 1, xb, rbits);
  // (measured: issuing block rb + 1's MFMAs before block rb's epilogue, two accumulator sets,
  // was ~5 % slower relative to the tile on the same box)
  for (int64_t rb = rb0; rb < rb1; rb += 2) {
    block(rb, xa, ra);
    if (rb + 1 < rb1) block(rb + 1, xb, rbits);
  }
}

// One launch: the instance <KS16, IL4, NT, ABL, 4, WL>.
struct SmallkArgs {
  int64_t M, N;
  int K;
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  const uint32_t *a_rows, *amax_b;
  const float* bias;
  int act;
  float* C;
  int64_t ldc;
  int n_slabs, chunk_blocks;
  hipStream_t st;
};
template <int KS16, bool IL4, bool NT, int ABL, bool WL>
int launch_smallk(unsigned blocks, const SmallkArgs& a, const char* what) {
  gemm_smallk_kernel<KS16, IL4, NT, ABL, 4, WL><<<blocks, 256, 0, a.st>>>(
      a.M, a.N, a.K, a.A, a.lda, a.B, a.ldb, a.a_rows, a.amax_b, a.bias, a.act, a.C, a.ldc, a.n_slabs,
      a.chunk_blocks);
  return check_launch(what);
}

}  // namespace

// Host: the shapes the small-K kernel takes (per-row A scales, K-contiguous B, K <= 96, every
// row and pointer 16-B aligned, N % 4 == 0, no beta, act 0 / 1).
bool smallk_fits(int b_kmajor, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                 const float* Bp, int64_t ldb, float beta, int act, const float* C, int64_t ldc) {
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  return option(MVML_OPT_SMALLK) != 0 && !b_kmajor && M > 0 && K >= 4 && K <= kSkMaxK && K % 4 == 0 &&
         N % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0 && al(A) && al(Bp) && al(C) &&
         beta == 0.f && (act == 0 || act == 1);
}

int smallk_launch(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B,
                  int64_t ldb, bool il4, const uint32_t* a_rows, const uint32_t* amax_b,
                  const float* bias, int act, float* C, int64_t ldc, hipStream_t st) {
  // 64 columns per wave (NG = 4).  Measured: 32-column slabs (NG = 2, 152 VGPRs, three waves
  // per SIMD) 3.38 vs 2.87 ms at config 3 — twice the A reads cost more than the occupancy buys
  const int n_slabs = (int)ceil_div(N, 64);
  const int64_t nrb = ceil_div(M, 16);
  // ~32 row blocks (512 rows) per wave: the B slab's one load is 1/30 of what the wave stores;
  // fewer on small launches so that >= 4096 waves fill the chip
  const int opt = option(MVML_OPT_SMALLK);
  const int64_t cap = opt == 3 ? 8 : (opt == 4 ? 128 : 32);  // (3 / 4: chunk-size variants)
  const int64_t cb = std::max<int64_t>(1, std::min<int64_t>(cap, nrb * n_slabs / 4096));
  const int64_t waves = ceil_div(nrb, cb) * n_slabs;
  const int64_t blocks = ceil_div(waves, 4);
  if (blocks >= (int64_t(1) << 31)) {
    set_error("gemm small-K: too many blocks");
    return MVML_ERR_INVALID;
  }
  const bool nt = opt != 2;  // (3 .. 6: timing variants)
  const int ks = (int)ceil_div(K, 16);  // 1 .. 6: the k-step plans above
  // WL: a workgroup = four row chunks of one slab
  const unsigned wl_blocks = (unsigned)(ceil_div(ceil_div(nrb, cb), 4) * n_slabs);
  const SmallkArgs a{M, N, (int)K, A, lda, B, ldb, a_rows, amax_b, bias, act, C, ldc, n_slabs, (int)cb, st};
  if (opt == 10 && ks == 5 && il4)  // (10: B fragments in registers — the round-5 first build)
    return launch_smallk<5, true, true, 0, false>((unsigned)blocks, a, "gemm_smallk_kernel(B in registers)");
  if ((opt == 5 || opt == 6) && ks == 5 && il4)
    return opt == 5 ? launch_smallk<5, true, true, 1, true>(wl_blocks, a, "gemm_smallk_kernel(ablation)")
                    : launch_smallk<5, true, true, 2, true>(wl_blocks, a, "gemm_smallk_kernel(ablation)");
  // the product: every k-step plan with B from its il4 image or fp32, non-temporal C stores or not
  return switch_const<1, 2, 3, 4, 5, 6>(std::min(ks, 6), [&](auto KS) {
    constexpr int ks16 = decltype(KS)::value;
    if (il4)
      return nt ? launch_smallk<ks16, true, true, 0, true>(wl_blocks, a, "gemm_smallk_kernel")
                : launch_smallk<ks16, true, false, 0, true>(wl_blocks, a, "gemm_smallk_kernel");
    return nt ? launch_smallk<ks16, false, true, 0, true>(wl_blocks, a, "gemm_smallk_kernel")
              : launch_smallk<ks16, false, false, 0, true>(wl_blocks, a, "gemm_smallk_kernel");
  });
}

}  // namespace mvml
