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

// column loaders of tuple_sums (below): K arrays as they are, or each behind a leading zero (the
// exclusive offsets and the total of every column, as shifted_input gives for one array); a null
// array is a column of zeros
template <int K, bool SHIFT>
struct ArrayColumns {
  const int64_t* p[K];
  __host__ __device__ int64_t operator()(int q, int64_t i) const {
    if (!p[q]) return 0;
    if (SHIFT) return i > 0 ? p[q][i - 1] : 0;
    return p[q][i];
  }
};

// The input 0, src[0], src[1], ..: an inclusive sum of its first n + 1 values is the exclusive
// offsets of src[0, n) with the total behind them (dst[0] = 0 .. dst[n]), in one scan and with no
// fill of the leading zero.
template <class T>
struct ShiftedLoad {
  const T* src;
  __host__ __device__ T operator()(int64_t i) const { return i > 0 ? src[i - 1] : T(0); }
};
template <class T>
using ShiftedInput = hipcub::TransformInputIterator<T, ShiftedLoad<T>, hipcub::CountingInputIterator<int64_t>>;
template <class T>
ShiftedInput<T> shifted_input(const T* src) {
  return ShiftedInput<T>(hipcub::CountingInputIterator<int64_t>(0), ShiftedLoad<T>{src});
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

// ---- K inclusive sums over the same n in ONE scan: the sums of a K-tuple.  Column q of element
// i comes from a loader, load(q, i) -> int64; its running sum goes to out[q][i] (a null out[q]
// drops the column).  Integer sums: the same values as K separate scans, in two launches
// instead of 2 K.
template <int K>
struct TupleK {
  int64_t v[K];
};
template <int K>
struct TupleAdd {
  __host__ __device__ TupleK<K> operator()(const TupleK<K>& a, const TupleK<K>& b) const {
    TupleK<K> r;
    for (int q = 0; q < K; ++q) r.v[q] = a.v[q] + b.v[q];
    return r;
  }
};
template <int K, class Load>
struct TupleLoad {
  Load load;
  __host__ __device__ TupleK<K> operator()(int64_t i) const {
    TupleK<K> r;
    for (int q = 0; q < K; ++q) r.v[q] = load(q, i);
    return r;
  }
};
// the output side: an iterator whose references store a tuple's columns into K arrays
template <int K>
struct TupleOut {
  int64_t* out[K];
  int64_t at;
  struct Ref {
    int64_t* out[K];
    int64_t i;
    __host__ __device__ const Ref& operator=(const TupleK<K>& x) const {
      for (int q = 0; q < K; ++q)
        if (out[q]) out[q][i] = x.v[q];
      return *this;
    }
  };
  using iterator_category = std::random_access_iterator_tag;
  using value_type = TupleK<K>;
  using difference_type = int64_t;
  using pointer = void;
  using reference = Ref;
  __host__ __device__ Ref operator[](int64_t n) const {
    Ref r;
    for (int q = 0; q < K; ++q) r.out[q] = out[q];
    r.i = at + n;
    return r;
  }
  __host__ __device__ Ref operator*() const { return (*this)[0]; }
  __host__ __device__ TupleOut operator+(int64_t n) const {
    TupleOut r = *this;
    r.at += n;
    return r;
  }
  __host__ __device__ TupleOut& operator+=(int64_t n) {
    at += n;
    return *this;
  }
};
template <int K, class Load>
using TupleInput = hipcub::TransformInputIterator<TupleK<K>, TupleLoad<K, Load>, hipcub::CountingInputIterator<int64_t>>;

// ws.p null: the size query (into ws->bytes); else the scan
template <int K, class Load>
int tuple_sums(Workspace* ws, Load load, int64_t* const (&out)[K], int n, hipStream_t stream, std::string* err) {
  TupleInput<K, Load> in(hipcub::CountingInputIterator<int64_t>(0), TupleLoad<K, Load>{load});
  TupleOut<K> o{};
  for (int q = 0; q < K; ++q) o.out[q] = out[q];
  o.at = 0;
  HIPCHK(hipcub::DeviceScan::InclusiveScan(ws->p, ws->bytes, in, o, TupleAdd<K>(), n, stream));
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
