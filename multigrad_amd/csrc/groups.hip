// Group gather and segment sum for user-written hierarchical models (ops/groups.py): the
// broadcast of per-group parameters to their objects, and its transpose.
//
// Gather     : out_c[i] = v_c[id[i]] for up to 4 columns per launch; grid-stride over quads
//              of objects, one 16-byte load of four ids and one 16-byte store per column.
// Segment sum: out_c[g] = sum of x_c over the objects of group g, as a reduce-by-key over the
//              objects in sorted order (the sort is done once, when the plan is built).  Every
//              workgroup owns fixed chunks of kChunk consecutive sorted positions.  In a
//              chunk: a sequential segmented scan of each thread's four entries, a segmented
//              Hillis-Steele scan over the 64 lanes, a fold of the wave aggregates in LDS.
//              A run that begins and ends inside the chunk is stored to out[g] by the thread
//              that holds its last entry.  A run that crosses a chunk edge leaves a partial in
//              one of the chunk's two carry slots (2c: the run entering from the left, 2c+1:
//              the run leaving to the right; a run that covers the whole chunk fills 2c and
//              puts an exact 0 into 2c+1, an unused slot holds key -1).  The carry list is
//              itself a list of (key, value) entries in which equal keys are adjacent, so the
//              same kernel reduces it, level after level, until one chunk remains: at most 4
//              launches below 2^31 objects, a depth of O(log N) additions for any group size.
//              A workgroup issues the loads of its next chunk before it reduces the current one.
// No float atomics and no data-dependent order: for a given plan and device the result is
// bitwise reproducible.  Groups without objects keep the 0 of the zero-filled output.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <vector>

#include "common.h"
#include "smf_host.h"
#include "sweep_host.h"

namespace mg {

namespace {

constexpr int kGrpThreads = 256;
constexpr int kGrpCols = 4;                  // operands per launch
constexpr int kChunk = kGrpThreads * 4;      // sorted positions per chunk (ops.groups.CHUNK)
constexpr int kGrpWaves = kGrpThreads / kWave;
constexpr int kKeyNone = -1;                 // an unused carry slot
constexpr int kKeyPast = -2;                 // a position beyond the list
constexpr int kKeyEdge = -3;                 // the neighbour of the first / last entry

template <auto Kernel>
int64_t chip_blocks() {
  static int64_t cap = resident_blocks(reinterpret_cast<const void*>(Kernel), kGrpThreads);
  return cap;
}

struct GatherArgs {
  const int* id;  // [n] group of every object, each in [0, G)
  const float* v[kGrpCols];  // [G] each
  float* out[kGrpCols];      // [n] each, 16-byte aligned
  int64_t n;
  int vec;  // id is 16-byte aligned
};

template <int NC>
__global__ __launch_bounds__(kGrpThreads) void group_gather_kernel(GatherArgs a) {
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kGrpThreads;
  for (int64_t q = (int64_t)blockIdx.x * kGrpThreads + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q * 4;
    if (a.vec && i0 + 4 <= a.n) {
      const int4 g = *reinterpret_cast<const int4*>(a.id + i0);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        *reinterpret_cast<float4*>(a.out[c] + i0) =
            make_float4(a.v[c][g.x], a.v[c][g.y], a.v[c][g.z], a.v[c][g.w]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + j;
        if (i < a.n) {
          const int g = a.id[i];
#pragma unroll
          for (int c = 0; c < NC; ++c) a.out[c][i] = a.v[c][g];
        }
      }
    }
  }
}

struct SegArgs {
  const int* key;   // [m] keys with equal keys adjacent; negative keys are never stored
  const int* perm;  // level 0 of a permuted plan: entry j is x[perm[j]]; else nullptr
  const float* x[kGrpCols];  // [m] each (level 0 of a permuted plan: [n], read through perm)
  float* out[kGrpCols];      // [G] each
  int* ckey;        // [2 * nchunks] carry keys of the next level; nullptr on the last level
  float* cval[kGrpCols];     // [2 * nchunks] carry values per column
  int64_t m;
  int64_t nchunks;
  int vec;  // key, perm and every x are 16-byte aligned
};

template <int NC>
__device__ __forceinline__ void put_carry(const SegArgs& a, int64_t slot, int key,
                                          const float (&val)[NC], bool zero) {
  if (a.ckey == nullptr) return;
  a.ckey[slot] = key;
#pragma unroll
  for (int c = 0; c < NC; ++c) a.cval[c][slot] = zero ? 0.0f : val[c];
}

// One thread's share of a chunk: four consecutive entries, and on the first / last lane of a
// wave the key of the entry before / after them.
template <int NC>
struct SegTile {
  int k[4];
  int kprev, knext;
  float v[NC][4];
};

// All global reads of a chunk.  They are issued one chunk ahead of their use (the loop below),
// so that they overlap the reduction of the chunk before.
template <int NC>
__device__ __forceinline__ void seg_load(const SegArgs& a, int64_t chunk, SegTile<NC>& t) {
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int64_t p0 = chunk * kChunk + (int64_t)tid * 4;
  // uniform over the workgroup: every chunk but a partial last one takes the 16-byte loads
  const bool full = a.vec && (chunk + 1) * kChunk <= a.m;
  if (a.perm != nullptr) {
    int src[4];
    if (full) {
      const int4 sv = *reinterpret_cast<const int4*>(a.perm + p0);
      src[0] = sv.x; src[1] = sv.y; src[2] = sv.z; src[3] = sv.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) src[j] = p0 + j < a.m ? a.perm[p0 + j] : -1;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) t.v[c][j] = src[j] >= 0 ? a.x[c][src[j]] : 0.0f;
  } else if (full) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float4 xv = *reinterpret_cast<const float4*>(a.x[c] + p0);
      t.v[c][0] = xv.x; t.v[c][1] = xv.y; t.v[c][2] = xv.z; t.v[c][3] = xv.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) t.v[c][j] = p0 + j < a.m ? a.x[c][p0 + j] : 0.0f;
  }
  if (full) {
    const int4 kv = *reinterpret_cast<const int4*>(a.key + p0);
    t.k[0] = kv.x; t.k[1] = kv.y; t.k[2] = kv.z; t.k[3] = kv.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) t.k[j] = p0 + j < a.m ? a.key[p0 + j] : kKeyPast;
  }
  // neighbours across a wave edge (inside a wave they come from a lane shuffle); they may lie
  // in the next or the previous chunk
  t.kprev = t.knext = kKeyEdge;
  if (lane == 0)
    t.kprev = p0 > 0 && p0 - 1 < a.m ? a.key[p0 - 1] : kKeyEdge;
  if (lane == kWave - 1)
    t.knext = p0 + 4 < a.m ? a.key[p0 + 4] : kKeyEdge;
}

template <int NC>
__global__ __launch_bounds__(kGrpThreads) void segment_sum_kernel(SegArgs a) {
  __shared__ float wave_val[NC][kGrpWaves];
  __shared__ int wave_head[kGrpWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = tid >> 6;
  SegTile<NC> t, ahead;
  if ((int64_t)blockIdx.x < a.nchunks) seg_load<NC>(a, blockIdx.x, t);
  for (int64_t chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x) {
    const bool more = chunk + gridDim.x < a.nchunks;
    if (more) seg_load<NC>(a, chunk + gridDim.x, ahead);
    const int (&k)[4] = t.k;
    const float (&v)[NC][4] = t.v;
    int kprev = __shfl_up(k[3], 1, kWave);
    int knext = __shfl_down(k[0], 1, kWave);
    if (lane == 0) kprev = t.kprev;
    if (lane == kWave - 1) knext = t.knext;
    bool hd[4], tl[4];  // entry j begins / ends a run
    hd[0] = k[0] != kprev;
    tl[3] = k[3] != knext;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      hd[j] = k[j] != k[j - 1];
      tl[j - 1] = hd[j];
    }
    // registers: s[c][j] = sum of the run of entry j over this thread's entries 0..j
    float s[NC][4];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      s[c][0] = v[c][0];
#pragma unroll
      for (int j = 1; j < 4; ++j) s[c][j] = hd[j] ? v[c][j] : s[c][j - 1] + v[c][j];
    }
    // lanes: inclusive segmented scan of (a head in this thread, the sum of its last run)
    int f = hd[0] | hd[1] | hd[2] | hd[3];
    float agg[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) agg[c] = s[c][3];
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int fo = __shfl_up(f, off, kWave);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float ao = __shfl_up(agg[c], off, kWave);
        if (lane >= off && !f) agg[c] += ao;
      }
      if (lane >= off) f |= fo;
    }
    int ef = __shfl_up(f, 1, kWave);  // the lanes before this one in the wave
    float ea[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) ea[c] = __shfl_up(agg[c], 1, kWave);
    if (lane == 0) {
      ef = 0;
#pragma unroll
      for (int c = 0; c < NC; ++c) ea[c] = 0.0f;
    }
    if (lane == kWave - 1) {
      wave_head[wid] = f;
#pragma unroll
      for (int c = 0; c < NC; ++c) wave_val[c][wid] = agg[c];
    }
    __syncthreads();
    // LDS: the run that enters this wave, folded over the waves before it in a fixed order
    int pf = 0;
    float pa[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) pa[c] = 0.0f;
    for (int w = 0; w < wid; ++w) {
      const int wf = wave_head[w];
#pragma unroll
      for (int c = 0; c < NC; ++c) pa[c] = wf ? wave_val[c][w] : pa[c] + wave_val[c][w];
      pf |= wf;
    }
    // what the entries before this thread add to its first run, and whether that run began
    // inside the chunk
    float inc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) inc[c] = ef ? ea[c] : pa[c] + ea[c];
    const bool inc_head = ef || pf;
    const int64_t slot = chunk * 2;
    bool seen = false;  // a head among this thread's entries 0..j
    float tot[NC];
    bool closed = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      seen = seen || hd[j];
#pragma unroll
      for (int c = 0; c < NC; ++c) tot[c] = seen ? s[c][j] : inc[c] + s[c][j];
      closed = seen || inc_head;
      if (tl[j]) {
        if (!closed) {
          put_carry<NC>(a, slot, k[j], tot, false);  // the run entering from the left ends here
        } else if (k[j] >= 0) {
#pragma unroll
          for (int c = 0; c < NC; ++c) a.out[c][k[j]] = tot[c];
        }
      }
    }
    if (tid == 0 && hd[0]) put_carry<NC>(a, slot, kKeyNone, tot, true);
    if (tid == kGrpThreads - 1) {  // tot / closed describe the chunk's last entry
      if (tl[3]) {
        put_carry<NC>(a, slot + 1, kKeyNone, tot, true);
      } else if (closed) {
        put_carry<NC>(a, slot + 1, k[3], tot, false);
      } else {  // one run covers the whole chunk
        put_carry<NC>(a, slot, k[3], tot, false);
        put_carry<NC>(a, slot + 1, k[3], tot, true);
      }
    }
    __syncthreads();  // wave_val / wave_head are reused by the next chunk
    if (more) t = ahead;
  }
}

void check_cols(const std::vector<torch::Tensor>& cols, int64_t numel, const char* what) {
  TORCH_CHECK(!cols.empty(), what, ": at least one operand");
  for (const auto& t : cols) {
    check_dev(t, what, at::kFloat);
    TORCH_CHECK(t.numel() == numel, what, ": operand has ", t.numel(), " elements, expected ",
                numel);
  }
}

template <int NC>
void launch_segment_level(const SegArgs& a, hipStream_t stream) {
  const int64_t blocks = std::min(a.nchunks, chip_blocks<segment_sum_kernel<NC>>());
  hipLaunchKernelGGL(segment_sum_kernel<NC>, dim3(blocks), dim3(kGrpThreads), 0, stream, a);
}

#define MG_DISPATCH_COLS(NCOLS, ...)                       \
  switch (NCOLS) {                                         \
    case 1: { constexpr int NC = 1; __VA_ARGS__; break; }  \
    case 2: { constexpr int NC = 2; __VA_ARGS__; break; }  \
    case 3: { constexpr int NC = 3; __VA_ARGS__; break; }  \
    default: { constexpr int NC = 4; __VA_ARGS__; break; } \
  }

}  // namespace

int64_t group_chunk() { return kChunk; }

// out_c = values_c[ids] for every operand; ids is the plan's int32 copy, range-checked when the
// plan was built.
std::vector<torch::Tensor> group_gather(torch::Tensor ids, std::vector<torch::Tensor> values,
                                        int64_t num_groups) {
  check_dev(ids, "ids", at::kInt);
  check_cols(values, num_groups, "group_gather");
  const int64_t n = ids.numel();
  TORCH_CHECK(n > 0 && n < (int64_t(1) << 31), "group_gather: 0 < N < 2^31 required");
  auto stream = at::hip::getCurrentHIPStream();
  std::vector<torch::Tensor> outs;
  const int64_t need = ((n + 3) / 4 + kGrpThreads - 1) / kGrpThreads;
  for (size_t b = 0; b < values.size(); b += kGrpCols) {
    const int nc = (int)std::min<size_t>(kGrpCols, values.size() - b);
    GatherArgs a;
    a.id = ids.data_ptr<int>();
    a.n = n;
    a.vec = aligned16(a.id);
    for (int c = 0; c < kGrpCols; ++c) {
      a.v[c] = nullptr;
      a.out[c] = nullptr;
    }
    for (int c = 0; c < nc; ++c) {
      outs.push_back(torch::empty({n}, values[b + c].options()));
      a.v[c] = values[b + c].data_ptr<float>();
      a.out[c] = outs.back().data_ptr<float>();
      a.vec = a.vec && aligned16(a.out[c]);
    }
    MG_DISPATCH_COLS(nc, {
      const int64_t blocks = std::min(need, chip_blocks<group_gather_kernel<NC>>());
      hipLaunchKernelGGL(group_gather_kernel<NC>, dim3(blocks), dim3(kGrpThreads), 0, stream, a);
    });
  }
  return outs;
}

// out_c[g] = sum of x_c over the objects of group g.  sorted_ids are the plan's ids in sorted
// order; perm (optional) maps a sorted position to its object, for a plan whose index was not
// already sorted.
std::vector<torch::Tensor> group_segment_sum(torch::Tensor sorted_ids,
                                             c10::optional<torch::Tensor> perm,
                                             std::vector<torch::Tensor> x, int64_t num_groups) {
  check_dev(sorted_ids, "sorted_ids", at::kInt);
  const int64_t n = sorted_ids.numel();
  TORCH_CHECK(n > 0 && n < (int64_t(1) << 31), "group_segment_sum: 0 < N < 2^31 required");
  TORCH_CHECK(num_groups > 0, "group_segment_sum: num_groups must be positive");
  check_cols(x, n, "group_segment_sum");
  const int* perm_ptr = nullptr;
  if (perm.has_value() && perm->defined()) {
    check_dev(*perm, "perm", at::kInt);
    TORCH_CHECK(perm->numel() == n, "perm must have N elements");
    perm_ptr = perm->data_ptr<int>();
  }
  auto stream = at::hip::getCurrentHIPStream();
  const auto fopt = x[0].options();
  const auto iopt = sorted_ids.options();
  std::vector<torch::Tensor> outs;
  for (size_t b = 0; b < x.size(); b += kGrpCols) {
    const int nc = (int)std::min<size_t>(kGrpCols, x.size() - b);
    SegArgs a;
    for (int c = 0; c < kGrpCols; ++c) {
      a.x[c] = nullptr;
      a.out[c] = nullptr;
      a.cval[c] = nullptr;
    }
    a.key = sorted_ids.data_ptr<int>();
    a.perm = perm_ptr;
    a.m = n;
    a.vec = aligned16(a.key) && (perm_ptr == nullptr || aligned16(perm_ptr));
    for (int c = 0; c < nc; ++c) {
      outs.push_back(torch::zeros({num_groups}, fopt));
      a.out[c] = outs.back().data_ptr<float>();
      a.x[c] = x[b + c].data_ptr<float>();
      if (perm_ptr == nullptr) a.vec = a.vec && aligned16(a.x[c]);
    }
    torch::Tensor ckey, cval;  // keep the level's inputs alive until its launch is enqueued
    for (;;) {
      a.nchunks = (a.m + kChunk - 1) / kChunk;
      torch::Tensor nkey, nval;
      int64_t cstride = 0;
      if (a.nchunks > 1) {
        cstride = (2 * a.nchunks + 3) / 4 * 4;  // columns stay 16-byte aligned
        nkey = torch::empty({2 * a.nchunks}, iopt);
        nval = torch::empty({(int64_t)nc, cstride}, fopt);
        a.ckey = nkey.data_ptr<int>();
        for (int c = 0; c < nc; ++c) a.cval[c] = nval.data_ptr<float>() + c * cstride;
      } else {
        a.ckey = nullptr;
      }
      MG_DISPATCH_COLS(nc, launch_segment_level<NC>(a, stream));
      if (a.nchunks == 1) break;
      ckey = nkey;
      cval = nval;
      a.key = a.ckey;
      a.perm = nullptr;
      a.m = 2 * a.nchunks;
      a.vec = aligned16(a.key);
      for (int c = 0; c < nc; ++c) {
        a.x[c] = a.cval[c];
        a.vec = a.vec && aligned16(a.x[c]);
      }
    }
  }
  return outs;
}

}  // namespace mg
