// Device helpers shared by the wave-per-row kernels (gat_agg_*.hip, gatv2_agg.hip, the readouts):
// lane broadcasts, float4 arithmetic and access, per-head selects and the H-value all-reduce.
// All are forced inline, so a kernel's machine code does not depend on whether its helpers come
// from here or from its own file (tools/codeobj_diff.py compares them; DESIGN.md, "GATv2").
// Where two forms of one helper exist below, the difference is deliberate: each says why.
#pragma once
#include "common.h"

namespace mvml {

__device__ __forceinline__ float rl(float x, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}
__device__ __forceinline__ int rl(int x, int j) { return __builtin_amdgcn_readlane(x, j); }

// A wave re-reads what its own lanes stored: order the accesses.  Two scopes, not to be merged:
// wavefront: the stores went to LDS (batch_csr.hip's counters and cursors)
__device__ __forceinline__ void wave_sync_wavefront_scope() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// workgroup: some went to global memory and are read back from there (gatv2_agg.hip's spilled scores)
__device__ __forceinline__ void wave_sync_workgroup_scope() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : x * slope; }
__device__ __forceinline__ float elu(float x) { return x > 0.f ? x : expm1f(x); }

__device__ __forceinline__ float4 f4(float a) { return make_float4(a, a, a, a); }
__device__ __forceinline__ float4 fma4(float a, float4 z, float4 c) {
  return make_float4(fmaf(a, z.x, c.x), fmaf(a, z.y, c.y), fmaf(a, z.z, c.z), fmaf(a, z.w, c.w));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
// explicit roundings: with the device default -ffp-contract=fast the compiler would pick the
// contraction per call site, so kernels that promise the same dots bitwise could differ
__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmul_rn(a.x, b.x))));
}
// the contractable form (readout.hip, set2set.hip): no kernel compares these dots bitwise with
// another's, so the compiler is free to fuse them
__device__ __forceinline__ float dot4_contract(float4 a, float4 b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// a[h] of H wave-uniform per-head values, h per lane, as a select chain.  Two forms:
// by reference (gat_agg_fwd.hip, gat_agg_bwd.hip): the array stays in registers in every instance there
template <int H>
__device__ __forceinline__ float pick(const float (&a)[H], int h) {
  float r = a[0];
#pragma unroll
  for (int k = 1; k < H; ++k) r = (h == k) ? a[k] : r;
  return r;
}
// BY VALUE (gatv2_agg.hip): through a reference the compiler turns the select chain into one
// load from a selected address, which keeps the array in memory (LDS, or scratch where the
// head-mean instances' LDS rows leave no room)
template <int H>
struct HeadVals {
  float v[H];
};
template <int H>
__device__ __forceinline__ float pick(HeadVals<H> a, int h) {
  float r = a.v[0];
#pragma unroll
  for (int k = 1; k < H; ++k) r = (h == k) ? a.v[k] : r;
  return r;
}
template <int H>
__device__ __forceinline__ void add_at(float (&a)[H], int h, float v) {
#pragma unroll
  for (int k = 0; k < H; ++k) a[k] += (h == k) ? v : 0.f;
}

// All-reduce of H per-lane values over the 64 lanes in (H - 1) + (6 - log2 H) shuffles instead
// of 6 H: a butterfly that halves the value count per step (lanes with the mask bit set keep
// the upper half) and then finishes the single remaining value inside 64/H-lane groups.  After
// it, lane l holds the total of head ((l >> (6 - log2 H)) & (H - 1)); readlane broadcasts them.
template <int H>
struct HeadReduce {
  static constexpr int LOG = H == 1 ? 0 : H == 2 ? 1 : H == 4 ? 2 : 3;
  template <bool MAX>
  __device__ static __forceinline__ float op(float a, float b) { return MAX ? fmaxf(a, b) : a + b; }
  template <bool MAX>
  __device__ static __forceinline__ void all(float (&v)[H], int lane) {
    float w[H];
#pragma unroll
    for (int h = 0; h < H; ++h) w[h] = v[h];
    if constexpr (H >= 8) step<MAX, 8>(w, lane, 32);
    if constexpr (H >= 4) step<MAX, 4>(w, lane, 32 >> (LOG - 2));
    if constexpr (H >= 2) step<MAX, 2>(w, lane, 32 >> (LOG - 1));
#pragma unroll
    for (int m = 32 >> LOG; m >= 1; m >>= 1) w[0] = op<MAX>(w[0], __shfl_xor(w[0], m, 64));
#pragma unroll
    for (int h = 0; h < H; ++h)
      v[h] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w[0]), h << (6 - LOG)));
  }
  template <bool MAX, int N>
  __device__ static __forceinline__ void step(float (&w)[H], int lane, int mask) {
    const bool hi = (lane & mask) != 0;
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const float keep = hi ? w[i + N / 2] : w[i];
      const float send = hi ? w[i] : w[i + N / 2];
      w[i] = op<MAX>(keep, __shfl_xor(send, mask, 64));
    }
  }
};

// g_rst[v, col..col+3] (per-head gradient of rst) from the layer-output gradient.
__device__ __forceinline__ float4 grst_of(const float* __restrict__ g_out, const float* __restrict__ out,
                                          int64_t v, int col, int HF, int F, int H, int mode) {
  if (mode == 1) {  // mean over heads: torch mean backward = grad / H
    const float4 g = ld4(g_out + v * F + (col % F));
    const float inv = (float)H;
    return make_float4(g.x / inv, g.y / inv, g.z / inv, g.w / inv);
  }
  float4 g = ld4(g_out + v * HF + col);
  if (mode == 0) {  // ELU'(x) = 1 (x > 0) else exp(x) = out + 1 (torch elu_backward, is_result)
    const float4 o = ld4(out + v * HF + col);
    g.x *= o.x > 0.f ? 1.f : o.x + 1.f;
    g.y *= o.y > 0.f ? 1.f : o.y + 1.f;
    g.z *= o.z > 0.f ? 1.f : o.z + 1.f;
    g.w *= o.w > 0.f ? 1.f : o.w + 1.f;
  }
  return g;
}

}  // namespace mvml
