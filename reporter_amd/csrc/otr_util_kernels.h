// otr_util_kernels.h — the small index kernels more than one unit launches (otr_tiles.hip,
// otr_text.hip).  All templates, so every unit that includes this header may instantiate
// them and the library still links one copy of each instance.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace otr {

template <class T>
__global__ void k_iota(T* v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (T)i;
}

template <class T>
__global__ void k_gather_by(const T* src, const int32_t* idx, int64_t n, T* dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}

// stream compaction by an inclusive scan of 0/1 flags: out[pos[i] - 1] = in[i]
template <class T>
__global__ void k_scatter_flagged(const T* in, const int64_t* flag, const int64_t* pos, int64_t n, T* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) out[pos[i] - 1] = in[i];
}

// the same for the indices themselves: out[pos[i] - 1] = i (32- or 64-bit)
template <class Out>
__global__ void k_scatter_index(const int64_t* flag, const int64_t* pos, int64_t n, Out* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) out[pos[i] - 1] = (Out)i;
}

// The scalars the host reads after a stage, gathered into one record of 8-byte words: up to
// eight runs src[q][0, n[q]) stored back to back at dst.  dst is the matcher's pinned mailbox
// (mapped host memory: the host reads it after the stream wait, no copy operation at all) or a
// device slab that one copy brings over.  One block.
constexpr int kPostRuns = 8;
struct PostArgs {
  const unsigned long long* src[kPostRuns];
  int n[kPostRuns];
  unsigned long long* dst;
};
template <int RUNS = kPostRuns>
__global__ void k_post(PostArgs a) {
  int o = 0;
  for (int q = 0; q < RUNS; ++q) {
    for (int i = threadIdx.x; i < a.n[q]; i += blockDim.x) a.dst[o + i] = a.src[q][i];
    o += a.n[q];
  }
}

}  // namespace otr
