// Class map of the atom-feature rows (mvml_feat_classes) and the row gather that goes with it
// (mvml_gather_rows).
//
// The first GAT layer's input rows are featurizer vectors: one-hot blocks and a few small
// integers, a few hundred distinct rows among the 1.75 M atoms of a config-3 step.  Numbering them
// lets the layer project one row per class and the aggregation read that table from L2
// (gat_agg_common.h, MAP instances) instead of an [N, H F + R] projection from HBM.
//
// Four launches, integer atomics only, nothing read back:
//   1. init:   the hash table (kTab slots of "smallest atom index of the class", empty = kEmpty)
//   2. probe:  one thread per atom holds its row in registers, hashes it and walks the table from
//              its home slot: an empty slot is claimed by CAS; an occupied one is compared with the
//              occupant's WHOLE row (bit for bit — the hash only picks the start) and on a match
//              takes atomicMin of the atom indices; else the next slot.  A class therefore owns
//              exactly one slot (slots are never freed, so every row of the class walks the same
//              occupied prefix), and after the launch the slot holds the class's first atom.
//              cls[a] = the slot, for now.
//   3. rank:   one block sorts the <= kMaxFeatClasses occupied slots by first atom (a rank count):
//              class id = rank, so ids follow first occurrence whatever the schedule was; copies
//              the class rows to Xc and writes the count.
//   4. map:    cls[a] = class of its slot.
// More classes than the capacity: probe stops claiming (the table never fills: kTab is 4x the
// capacity and at most the threads in flight pass it, bounded by the walk length), rank writes
// capacity + 1 and zero classes, so every cls stays a valid row index whatever happened.
#include "common.h"

namespace mvml {
namespace {

constexpr int kMaxClasses = MVML_MAX_FEAT_CLASSES;
constexpr int kTab = 4 * kMaxClasses;
constexpr int kEmpty = 0x7FFFFFFF;
constexpr int kRowQ = MVML_FEAT_CLASS_MAX_LD / 4;  // 16-B pieces of the longest row
static_assert((kTab & (kTab - 1)) == 0, "the table size is a power of two");

// workspace (int32): slots [kTab] | slot class [kTab] | ctrl = {claimed slots, overflow}
struct ClassWs {
  int* slots;
  int* slot_cls;
  int* ctrl;
  explicit ClassWs(void* p) : slots(static_cast<int*>(p)), slot_cls(slots + kTab), ctrl(slots + 2 * kTab) {}
};

__global__ void __launch_bounds__(256) feat_class_init_kernel(int* slots, int* ctrl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kTab) slots[i] = kEmpty;
  if (i < 2) ctrl[i] = 0;
}

__device__ __forceinline__ uint4 ldrow(const float* X, int64_t row, int64_t ldx, int j) {
  return *reinterpret_cast<const uint4*>(X + row * ldx + 4 * j);
}

__global__ void __launch_bounds__(256)
feat_class_probe_kernel(int64_t N, const float* __restrict__ X, int64_t ldx, int* slots, int* ctrl,
                        int32_t* __restrict__ cls) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a >= N) return;
  const int q = (int)(ldx / 4);
  uint4 r[kRowQ];
  uint32_t h = 2166136261u;
#pragma unroll
  for (int j = 0; j < kRowQ; ++j) {
    r[j] = j < q ? ldrow(X, a, ldx, j) : make_uint4(0, 0, 0, 0);
    h = (h ^ r[j].x) * 16777619u;
    h = (h ^ r[j].y) * 16777619u;
    h = (h ^ r[j].z) * 16777619u;
    h = (h ^ r[j].w) * 16777619u;
  }
  h ^= h >> 15;
  int s = (int)(h & (kTab - 1));
  for (int it = 0; it < kTab; ++it, s = (s + 1) & (kTab - 1)) {
    if (__atomic_load_n(&ctrl[1], __ATOMIC_RELAXED)) break;  // over capacity: no map this time
    int cur = __atomic_load_n(&slots[s], __ATOMIC_RELAXED);
    if (cur == kEmpty) {
      cur = atomicCAS(&slots[s], kEmpty, (int)a);
      if (cur == kEmpty) {  // a new class
        if (atomicAdd(&ctrl[0], 1) >= kMaxClasses) atomicExch(&ctrl[1], 1);
        cls[a] = s;
        return;
      }
    }
    // the occupant (any atom of its class: atomicMin only swaps equal rows): whole-row compare
    bool eq = true;
#pragma unroll
    for (int j = 0; j < kRowQ; ++j)
      if (j < q) {
        const uint4 t = ldrow(X, cur, ldx, j);
        eq = eq && t.x == r[j].x && t.y == r[j].y && t.z == r[j].z && t.w == r[j].w;
      }
    if (eq) {
      if (a < cur) atomicMin(&slots[s], (int)a);
      cls[a] = s;
      return;
    }
  }
  cls[a] = 0;
}

__global__ void __launch_bounds__(1024)
feat_class_rank_kernel(const float* __restrict__ X, int64_t ldx, const int* __restrict__ slots,
                       int* __restrict__ slot_cls, const int* __restrict__ ctrl, float* __restrict__ Xc,
                       int32_t* __restrict__ count) {
  __shared__ int s_rep[kMaxClasses], s_slot[kMaxClasses];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  if (ctrl[1] || ctrl[0] > kMaxClasses) {
    for (int s = tid; s < kTab; s += 1024) slot_cls[s] = 0;
    if (tid == 0) *count = kMaxClasses + 1;
    return;
  }
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int s = tid; s < kTab; s += 1024) {
    const int rep = slots[s];
    slot_cls[s] = 0;
    if (rep != kEmpty) {
      const int i = atomicAdd(&s_n, 1);  // (the order of this list does not reach the result)
      s_rep[i] = rep;
      s_slot[i] = s;
    }
  }
  __syncthreads();
  const int n = s_n;
  if (tid == 0) *count = n;
  if (tid >= n) return;
  const int rep = s_rep[tid];
  int rank = 0;
  for (int j = 0; j < n; ++j) rank += s_rep[j] < rep ? 1 : 0;  // first atoms are distinct
  slot_cls[s_slot[tid]] = rank;
  for (int j = 0; j < (int)(ldx / 4); ++j)
    *reinterpret_cast<uint4*>(Xc + (int64_t)rank * ldx + 4 * j) = ldrow(X, rep, ldx, j);
}

__global__ void __launch_bounds__(256)
feat_class_map_kernel(int64_t N, const int* __restrict__ slot_cls, int32_t* __restrict__ cls) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a < N) cls[a] = slot_cls[cls[a] & (kTab - 1)];
}

// one thread per piece of V floats (V = 4: 16-B pieces; 1: any width and alignment)
template <typename T>
__global__ void __launch_bounds__(256)
gather_rows_kernel(int64_t rows, int pieces, const float* __restrict__ src, int64_t lds,
                   const int32_t* __restrict__ idx, float* __restrict__ dst, int64_t ldd) {
  constexpr int V = sizeof(T) / sizeof(float);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * pieces) return;
  const int64_t r = i / pieces;
  const int c = (int)(i % pieces);
  *reinterpret_cast<T*>(dst + r * ldd + V * c) = *reinterpret_cast<const T*>(src + (int64_t)idx[r] * lds + V * c);
}

}  // namespace
}  // namespace mvml

using namespace mvml;

extern "C" size_t mvml_feat_classes_workspace_size(void) { return carve_size((2 * kTab + 2) * sizeof(int)); }

extern "C" int mvml_feat_classes(int64_t num_rows, const float* X, int64_t ldx, int32_t* cls, float* Xc,
                                 int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  MVML_REQUIRE(num_rows >= 0 && num_rows < (int64_t(1) << 31), "feat_classes: bad row count");
  MVML_REQUIRE(ldx >= 4 && ldx % 4 == 0 && ldx <= MVML_FEAT_CLASS_MAX_LD,
               "feat_classes: ldx must be a multiple of 4 in [4, %d] (got %lld)", MVML_FEAT_CLASS_MAX_LD,
               (long long)ldx);
  MVML_REQUIRE(Xc && aligned16(Xc) && count && (num_rows == 0 || (X && aligned16(X) && cls)),
               "feat_classes: X / Xc must be 16-byte aligned, cls and count given");
  if (!workspace || workspace_bytes < mvml_feat_classes_workspace_size()) {
    set_error("feat_classes: workspace of mvml_feat_classes_workspace_size() bytes required");
    return MVML_ERR_WORKSPACE;
  }
  const ClassWs w(workspace);
  hipStream_t st = as_stream(stream);
  feat_class_init_kernel<<<kTab / 256, 256, 0, st>>>(w.slots, w.ctrl);
  int rc = check_launch("feat_class_init_kernel");
  if (rc) return rc;
  const unsigned blocks = (unsigned)ceil_div(num_rows, 256);
  if (num_rows > 0) {
    feat_class_probe_kernel<<<blocks, 256, 0, st>>>(num_rows, X, ldx, w.slots, w.ctrl, cls);
    if ((rc = check_launch("feat_class_probe_kernel"))) return rc;
  }
  feat_class_rank_kernel<<<1, 1024, 0, st>>>(X, ldx, w.slots, w.slot_cls, w.ctrl, Xc, count);
  if ((rc = check_launch("feat_class_rank_kernel"))) return rc;
  if (num_rows > 0) {
    feat_class_map_kernel<<<blocks, 256, 0, st>>>(num_rows, w.slot_cls, cls);
    if ((rc = check_launch("feat_class_map_kernel"))) return rc;
  }
  return MVML_OK;
}

extern "C" int mvml_gather_rows(int64_t rows, int cols, const float* src, int64_t lds, const int32_t* idx,
                                float* dst, int64_t ldd, void* stream) {
  clear_error();
  MVML_REQUIRE(rows >= 0 && cols > 0, "gather_rows: bad shape");
  if (rows == 0) return MVML_OK;
  MVML_REQUIRE(src && dst && idx && lds >= cols && ldd >= cols, "gather_rows: rows of cols floats at strides >= cols");
  const bool v4 = cols % 4 == 0 && row_ok(src, lds, cols) && row_ok(dst, ldd, cols);
  const int pieces = v4 ? cols / 4 : cols;
  const int64_t blocks = ceil_div(rows * pieces, 256);
  MVML_REQUIRE(blocks < (int64_t(1) << 31), "gather_rows: too many elements");
  if (v4) gather_rows_kernel<float4><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(rows, pieces, src, lds, idx, dst, ldd);
  else gather_rows_kernel<float><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(rows, pieces, src, lds, idx, dst, ldd);
  return check_launch("gather_rows_kernel");
}
