// torch.nn.GRUCell after its two gate products (AttentiveFP's AttentiveGRU1 / AttentiveGRU2 and the
// readout's GRUCell): gi = x Wih^T and gh = h Whh^T, both [M][3D] dense, are GEMM calls; this file
// adds both biases, applies the gates and (optionally) the ReLU that follows the two atom-level
// uses.  Gate order r, z, n (torch's weight_ih / weight_hh row blocks).
//
//   r = sig(gi_r + bih_r + gh_r + bhh_r)     z = sig(gi_z + bih_z + gh_z + bhh_z)
//   n = tanh(gi_n + bih_n + r (gh_n + bhh_n))          h' = (1 - z) n + z h
//
// Element-wise: one thread per float4 of the [M][D] rows, 64-bit indices (1.75 M atom rows x 200
// and 65,536 graph rows both run it).  The forward saves [r | z | n | gh_n + bhh_n] per row, so the
// backward reads neither gate product again; the ReLU's side comes from the output.
#include "common.h"
#include "wave_ops.h"

namespace mvml {
namespace {

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__global__ void __launch_bounds__(256)
gru_cell_fwd_kernel(int64_t M, int D, const float* __restrict__ gi, const float* __restrict__ gh,
                    const float* __restrict__ bih, const float* __restrict__ bhh, const float* __restrict__ h,
                    int64_t ldh, int relu, float* __restrict__ out, int64_t ldo, float* __restrict__ save) {
  const int q = D / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * q) return;
  const int64_t m = i / q;
  const int c = 4 * (int)(i - m * q);
  const float* gir = gi + m * 3 * D + c;
  const float* ghr = gh + m * 3 * D + c;
  const float4 ir = ld4(gir), iz = ld4(gir + D), in = ld4(gir + 2 * D);
  const float4 hr = ld4(ghr), hz = ld4(ghr + D), hn = ld4(ghr + 2 * D);
  const float4 bir = ld4(bih + c), biz = ld4(bih + D + c), bin = ld4(bih + 2 * D + c);
  const float4 bhr = ld4(bhh + c), bhz = ld4(bhh + D + c), bhn = ld4(bhh + 2 * D + c);
  const float4 hp = ld4(h + m * ldh + c);
  float r[4], z[4], n[4], g[4], o[4];
  const float a_ir[4] = {ir.x, ir.y, ir.z, ir.w}, a_iz[4] = {iz.x, iz.y, iz.z, iz.w}, a_in[4] = {in.x, in.y, in.z, in.w};
  const float a_hr[4] = {hr.x, hr.y, hr.z, hr.w}, a_hz[4] = {hz.x, hz.y, hz.z, hz.w}, a_hn[4] = {hn.x, hn.y, hn.z, hn.w};
  const float a_bir[4] = {bir.x, bir.y, bir.z, bir.w}, a_biz[4] = {biz.x, biz.y, biz.z, biz.w};
  const float a_bin[4] = {bin.x, bin.y, bin.z, bin.w}, a_bhr[4] = {bhr.x, bhr.y, bhr.z, bhr.w};
  const float a_bhz[4] = {bhz.x, bhz.y, bhz.z, bhz.w}, a_bhn[4] = {bhn.x, bhn.y, bhn.z, bhn.w};
  const float a_h[4] = {hp.x, hp.y, hp.z, hp.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r[k] = sigmoidf((a_ir[k] + a_bir[k]) + (a_hr[k] + a_bhr[k]));
    z[k] = sigmoidf((a_iz[k] + a_biz[k]) + (a_hz[k] + a_bhz[k]));
    g[k] = a_hn[k] + a_bhn[k];
    n[k] = tanhf((a_in[k] + a_bin[k]) + r[k] * g[k]);
    const float hv = (1.f - z[k]) * n[k] + z[k] * a_h[k];
    o[k] = relu ? (hv > 0.f ? hv : 0.f) : hv;
  }
  float* sv = save + m * 4 * D + c;
  st4(sv, make_float4(r[0], r[1], r[2], r[3]));
  st4(sv + D, make_float4(z[0], z[1], z[2], z[3]));
  st4(sv + 2 * D, make_float4(n[0], n[1], n[2], n[3]));
  st4(sv + 3 * D, make_float4(g[0], g[1], g[2], g[3]));
  st4(out + m * ldo + c, make_float4(o[0], o[1], o[2], o[3]));
}

__global__ void __launch_bounds__(256)
gru_cell_bwd_kernel(int64_t M, int D, const float* __restrict__ save, const float* __restrict__ h, int64_t ldh,
                    const float* __restrict__ out, int64_t ldo, const float* __restrict__ g_out, int64_t ldg, int relu,
                    float* __restrict__ g_gi, float* __restrict__ g_gh, float* __restrict__ g_h, int64_t ldgh) {
  const int q = D / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * q) return;
  const int64_t m = i / q;
  const int c = 4 * (int)(i - m * q);
  const float* sv = save + m * 4 * D + c;
  const float4 r4 = ld4(sv), z4 = ld4(sv + D), n4 = ld4(sv + 2 * D), gn4 = ld4(sv + 3 * D);
  const float4 h4 = ld4(h + m * ldh + c);
  float4 g4 = ld4(g_out + m * ldg + c);
  if (relu) {
    const float4 o = ld4(out + m * ldo + c);
    g4 = make_float4(o.x > 0.f ? g4.x : 0.f, o.y > 0.f ? g4.y : 0.f, o.z > 0.f ? g4.z : 0.f, o.w > 0.f ? g4.w : 0.f);
  }
  const float r[4] = {r4.x, r4.y, r4.z, r4.w}, z[4] = {z4.x, z4.y, z4.z, z4.w}, n[4] = {n4.x, n4.y, n4.z, n4.w};
  const float gn[4] = {gn4.x, gn4.y, gn4.z, gn4.w}, hp[4] = {h4.x, h4.y, h4.z, h4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w};
  float dr[4], dz[4], dn[4], dnr[4], dh[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    dn[k] = g[k] * (1.f - z[k]) * (1.f - n[k] * n[k]);  // at n's pre-activation
    dz[k] = g[k] * (hp[k] - n[k]) * z[k] * (1.f - z[k]);
    dr[k] = dn[k] * gn[k] * r[k] * (1.f - r[k]);
    dnr[k] = dn[k] * r[k];
    dh[k] = g[k] * z[k];
  }
  float* a = g_gi + m * 3 * D + c;
  float* b = g_gh + m * 3 * D + c;
  st4(a, make_float4(dr[0], dr[1], dr[2], dr[3]));
  st4(a + D, make_float4(dz[0], dz[1], dz[2], dz[3]));
  st4(a + 2 * D, make_float4(dn[0], dn[1], dn[2], dn[3]));
  st4(b, make_float4(dr[0], dr[1], dr[2], dr[3]));
  st4(b + D, make_float4(dz[0], dz[1], dz[2], dz[3]));
  st4(b + 2 * D, make_float4(dnr[0], dnr[1], dnr[2], dnr[3]));
  st4(g_h + m * ldgh + c, make_float4(dh[0], dh[1], dh[2], dh[3]));
}

inline int check_gru(const char* who, int64_t M, int D) {
  MVML_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024, "%s: D must be a positive multiple of 4 <= 1024 (got %d)", who, D);
  // (one thread per float4: the grid stays below 2^31 workgroups)
  MVML_REQUIRE(M >= 0 && M < (int64_t(1) << 36) && ceil_div(M * (D / 4), 256) < (int64_t(1) << 31), "%s: bad M %lld",
               who, (long long)M);
  return MVML_OK;
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" int mvml_gru_cell_fwd(int64_t M, int D, const float* gi, const float* gh, const float* b_ih,
                                 const float* b_hh, const float* h, int64_t ldh, int relu, float* out, int64_t ldo,
                                 float* save, void* stream) {
  clear_error();
  if (int rc = check_gru("gru_cell_fwd", M, D)) return rc;
  if (M == 0) return MVML_OK;
  MVML_REQUIRE(gi != nullptr && gh != nullptr && b_ih != nullptr && b_hh != nullptr && save != nullptr &&
                   aligned16(gi) && aligned16(gh) && aligned16(b_ih) && aligned16(b_hh) && aligned16(save),
               "gru_cell_fwd: gi, gh, b_ih, b_hh and save are required, 16-byte aligned");
  MVML_REQUIRE(row_ok(h, ldh, D) && row_ok(out, ldo, D),
               "gru_cell_fwd: h and out must be 16-byte aligned with pitches >= D that are multiples of 4");
  gru_cell_fwd_kernel<<<(unsigned)ceil_div(M * (D / 4), 256), 256, 0, as_stream(stream)>>>(
      M, D, gi, gh, b_ih, b_hh, h, ldh, relu, out, ldo, save);
  return check_launch("gru_cell_fwd_kernel");
}

extern "C" int mvml_gru_cell_bwd(int64_t M, int D, const float* save, const float* h, int64_t ldh, const float* out,
                                 int64_t ldo, const float* g_out, int64_t ldg, int relu, float* g_gi, float* g_gh,
                                 float* g_h, int64_t ldgh, void* stream) {
  clear_error();
  if (int rc = check_gru("gru_cell_bwd", M, D)) return rc;
  if (M == 0) return MVML_OK;
  MVML_REQUIRE(save != nullptr && g_gi != nullptr && g_gh != nullptr && aligned16(save) && aligned16(g_gi) &&
                   aligned16(g_gh),
               "gru_cell_bwd: save, g_gi and g_gh are required, 16-byte aligned");
  MVML_REQUIRE(row_ok(h, ldh, D) && row_ok(g_out, ldg, D) && row_ok(g_h, ldgh, D) && (!relu || row_ok(out, ldo, D)),
               "gru_cell_bwd: h, out, g_out and g_h must be 16-byte aligned with pitches >= D that are multiples of 4");
  gru_cell_bwd_kernel<<<(unsigned)ceil_div(M * (D / 4), 256), 256, 0, as_stream(stream)>>>(
      M, D, save, h, ldh, out, ldo, g_out, ldg, relu, g_gi, g_gh, g_h, ldgh);
  return check_launch("gru_cell_bwd_kernel");
}
