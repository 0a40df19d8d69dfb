// otr_devscan.h — the scan, sort and read-back steps of the host-side stages over hipcub
// (host code only).  hipcub works in two steps: a size query, then the call with a workspace
// of that size.  A stage sizes ONE workspace before its first launch, for its largest n and
// the larger of its scan and sort needs (scan_bytes, sort_bytes), and hands it to every
// inclusive_sum / sort_pairs of the call: nothing here allocates, so no workspace is freed or
// grown under kernels already queued.  pool_scan / pool_sort are the stores' way: a workspace
// slot of their pool per step.
#pragma once
#include <hipcub/hipcub.hpp>

#include "otr_hostdev.h"

namespace otr {

struct Workspace {
  void* p = nullptr;
  size_t bytes = 0;
};

// The pointer types are deduced, so a size query and its call name the same hipcub instance:
// give the query the arrays of the call (it reads only their types) or typed null pointers.

// the workspace an inclusive sum of in[0, n) into out needs
template <class In, class Out>
int scan_bytes(In in, Out out, int n, size_t* bytes, hipStream_t stream, std::string* err) {
  HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, *bytes, in, out, n, stream));
  return OTR_OK;
}

// the workspace a sort of n (key, value) pairs by key bits [begin_bit, end_bit) needs
template <class K, class V>
int sort_bytes(const K* k_in, K* k_out, const V* v_in, V* v_out, int n, int begin_bit, int end_bit, size_t* bytes,
               hipStream_t stream, std::string* err) {
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, k_in, k_out, v_in, v_out, n, begin_bit, end_bit, stream));
  return OTR_OK;
}

// the larger of the two: one workspace for a call that scans and sorts n elements at most
template <class In, class Out, class K, class V>
int scan_sort_bytes(In in, Out out, const K* k_in, K* k_out, const V* v_in, V* v_out, int n, size_t* bytes,
                    hipStream_t stream, std::string* err) {
  size_t scan = 0, sort = 0;
  if (int rc = scan_bytes(in, out, n, &scan, stream, err)) return rc;
  if (int rc = sort_bytes(k_in, k_out, v_in, v_out, n, 0, 8 * (int)sizeof(K), &sort, stream, err)) return rc;
  *bytes = std::max(scan, sort);
  return OTR_OK;
}

// out[i] = in[0] + .. + in[i]; ws of at least scan_bytes
template <class In, class Out>
int inclusive_sum(Workspace ws, In in, Out out, int n, hipStream_t stream, std::string* err) {
  HIPCHK(hipcub::DeviceScan::InclusiveSum(ws.p, ws.bytes, in, out, n, stream));
  return OTR_OK;
}

// stable radix sort of the pairs by key bits [begin_bit, end_bit); ws of at least sort_bytes
template <class K, class V>
int sort_pairs(Workspace ws, const K* k_in, K* k_out, const V* v_in, V* v_out, int n, int begin_bit, int end_bit,
               hipStream_t stream, std::string* err) {
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(ws.p, ws.bytes, k_in, k_out, v_in, v_out, n, begin_bit, end_bit, stream));
  return OTR_OK;
}

// the workspace taken from a pool slot for this one step (the pool grows it when it is too small)
template <class In, class Out>
int pool_scan(DevPool& pool, int slot, In in, Out out, int64_t n, hipStream_t stream, std::string* err) {
  Workspace ws;
  if (int rc = scan_bytes(in, out, (int)n, &ws.bytes, stream, err)) return rc;
  ws.p = pool.get<char>(slot, ws.bytes);
  return inclusive_sum(ws, in, out, (int)n, stream, err);
}

template <class K, class V>
int pool_sort(DevPool& pool, int slot, const K* k_in, K* k_out, const V* v_in, V* v_out, int64_t n, int begin_bit,
              int end_bit, hipStream_t stream, std::string* err) {
  Workspace ws;
  if (int rc = sort_bytes(k_in, k_out, v_in, v_out, (int)n, begin_bit, end_bit, &ws.bytes, stream, err)) return rc;
  ws.p = pool.get<char>(slot, ws.bytes);
  return sort_pairs(ws, k_in, k_out, v_in, v_out, (int)n, begin_bit, end_bit, stream, err);
}

// Scalars read back from the device, then ONE host wait for all of them:
//   read_back(stream, err, fetch(&n_runs, pos + (n - 1)), fetch(&bad, d_bad))
template <class T>
struct Fetch {
  T* host;
  const T* dev;
};
template <class T>
Fetch<T> fetch(T* host, const T* dev) {
  return Fetch<T>{host, dev};
}
template <class... T>
int read_back(hipStream_t stream, std::string* err, Fetch<T>... f) {
  hipError_t e = hipSuccess;
  ((e = e != hipSuccess ? e : hipMemcpyAsync(f.host, f.dev, sizeof(T), hipMemcpyDeviceToHost, stream)), ...);
  HIPCHK(e);
  HIPCHK(hipStreamSynchronize(stream));
  return OTR_OK;
}

}  // namespace otr
