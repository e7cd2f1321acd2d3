// Device code of the fused stage kernels (included by stage_launch.hpp and long_fft.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cassert>
#include <type_traits>

#include "gpu/gpu_runtime.hpp"
#include "kernels/fft_device.hpp"
#include "kernels/stage_args.hpp"
#include "fft/fft_plan.hpp"

namespace spfft {
namespace dev {

// Streaming global accesses: every stage reads and writes each element once, so
// loads and stores carry the non-temporal hint (measured on MI355X: 268 MB copy
// 6.15-6.28 TB/s with nt vs 5.65-5.88 TB/s without, tools/probes/hbm_copy.hip).
template <typename T>
__device__ __forceinline__ cx<T> ld_stream(const cx<T>* p) {
  using V = T __attribute__((ext_vector_type(2)));
  const V v = __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
  return mk<T>(v.x, v.y);
}
template <typename T>
__device__ __forceinline__ void st_stream(cx<T>* p, cx<T> v) {
  using V = T __attribute__((ext_vector_type(2)));
  V w;
  w.x = v.x;
  w.y = v.y;
  __builtin_nontemporal_store(w, reinterpret_cast<V*>(p));
}
// Stick-side accesses of the backward z -> y hand-off: streaming (nt), or with
// the default cache policy (Plain: the lines stay in the 256 MB Infinity
// Cache, where the y stage finds them; GpuExecutor::plainHandoff_). Plain is a
// template parameter of the kernels, not a run-time flag: with a run-time
// branch the compiler merged the two stores (loads) of the branch into one and
// dropped the non-temporal hint, so every stick access ran plain (512^3 R2C
// fp32 z backward 146 -> 206 us, z forward 112 -> 129 us; profiles/r6/ntmerge).
template <bool Plain, typename T>
__device__ __forceinline__ cx<T> ld_stick(const cx<T>* p) {
  if constexpr (Plain) return *p;
  else return ld_stream(p);
}
template <bool Plain, typename T>
__device__ __forceinline__ void st_stick(cx<T>* p, cx<T> v) {
  if constexpr (Plain) *p = v;
  else st_stream(p, v);
}
// The [z][column][y] intermediate is streamed like the rest.
template <typename T>
__device__ __forceinline__ cx<T> ld_inter(const cx<T>* p) {
  return ld_stream(p);
}
template <typename T>
__device__ __forceinline__ void st_inter(cx<T>* p, cx<T> v) {
  st_stream(p, v);
}
// Sparse frequency values: a stick's values rarely start on a cache-line
// boundary, so neighbouring workgroups share lines; plain accesses keep them.
template <typename T>
__device__ __forceinline__ cx<T> ld_values(const cx<T>* p) {
  return *p;
}
template <typename T>
__device__ __forceinline__ void st_values(cx<T>* p, cx<T> v) {
  *p = v;
}
template <typename T>
__device__ __forceinline__ T ld_stream_real(const T* p) {
  return __builtin_nontemporal_load(p);
}
template <typename T>
__device__ __forceinline__ void st_stream_real(T* p, T v) {
  __builtin_nontemporal_store(v, p);
}

// Loads issued per lane before the first dependent LDS store: keeps U global
// loads in flight per lane (memory-level parallelism for the gathers).
constexpr int kGatherUnroll = 16;

// for idx in [0, total): lds[dst(idx)] = load(idx) (dst < 0: skip), U loads in flight.
template <typename T, class Load, class Dst>
__device__ __forceinline__ void gather_to_lds(cx<T>* lds, int total, Load load, Dst dst) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kGatherUnroll) {
    cx<T> v[kGatherUnroll];
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) v[u] = load(idx);
    }
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const int d = dst(idx);
        if (d >= 0) lds[d] = v[u];
      }
    }
  }
}

// for idx in [0, total): st(idx, lds[src(idx)]), U LDS reads in flight per lane
// before the dependent global stores (a plain loop waits out the LDS latency of
// every element).
template <typename T, class Src, class St>
__device__ __forceinline__ void scatter_from_lds(const cx<T>* lds, int total, Src src, St st) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kGatherUnroll) {
    cx<T> v[kGatherUnroll];
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) v[u] = lds[src(idx)];
    }
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) st(idx, v[u]);
    }
  }
}


// LDS -> global copy-out of a stage kernel: the run-time engines batch their LDS
// reads (scatter_from_lds, measured +5-7% at 100^3-240^3); the compile-time
// engines keep the plain loop (batching measured 1-2% slower at 128^3-256^3).
// A full tile of a compile-time engine (every line present) copies with a
// fully unrolled loop of compile-time trip count E: its LDS reads issue back to
// back instead of one read, wait and store per iteration.
template <class Eng, typename T, class Src, class St>
__device__ __forceinline__ void copy_out(const cx<T>* lds, int total, Src src, St st) {
  if constexpr (Eng::kBatchedCopy) {
    scatter_from_lds(lds, total, src, st);
  } else {
    using F = typename Eng::F;
    // (mixed-radix shapes can leave lanes idle: their tiles need not split evenly)
    constexpr bool kEven = (F::B * Eng::kN) % F::NT == 0;
    if (kEven && total == F::B * Eng::kN) {
      constexpr int kIters = kEven ? F::B * Eng::kN / F::NT : 1;
      cx<T> v[kIters];
#pragma unroll
      for (int i = 0; i < kIters; ++i) v[i] = lds[src(static_cast<int>(threadIdx.x) + i * F::NT)];
#pragma unroll
      for (int i = 0; i < kIters; ++i) st(static_cast<int>(threadIdx.x) + i * F::NT, v[i]);
      return;
    }
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) st(idx, lds[src(idx)]);
  }
}

// ------------------------------------------------------------ engine adapters
// TwPre: the FftCT twiddle prefetch (off for the kernels where its registers
// cost occupancy: the fp32 y forward kernels measured 61 -> 65 us at 256^3 and
// 260 -> 384 us at 512^3 with it, 129+ VGPRs, one 512-thread workgroup per CU)
// SS: direction of the engine shape (FftCT); CtEng is the engine of a stage
// with the shape of its own direction.
template <typename T, int N, int S, bool LF, bool TwPre, int SS>
struct CtEngS {
  using F = typename CtCore<T, N, S, LF, TwPre, SS>::type;
  static constexpr int kN = N;
  static constexpr bool kBatchedCopy = false;
  static constexpr bool kLineFast = LF;
  static constexpr int kBlock = F::NT > kMaxThreads ? F::NT : kMaxThreads;
  __device__ __forceinline__ int lines() const { return F::B; }
  __device__ __forceinline__ int n() const { return N; }
  __device__ __forceinline__ int in_at(int b, int pos) const { return F::in_at(b, pos); }
  __device__ __forceinline__ int out_at(int b, int pos) const { return F::out_at(b, pos); }
  __device__ __forceinline__ int input_elems() const { return F::B * F::LS; }
  __device__ __forceinline__ int lds_bytes() const { return static_cast<int>(F::lds_bytes()); }
  template <class St>
  __device__ __forceinline__ void lds_to_global(cx<T>* lds, const cx<T>* __restrict__ tw, St st) const {
    F::run(lds, tw, NoLoad{}, st);
  }
  template <class Ld>
  __device__ __forceinline__ void global_to_lds(cx<T>* lds, const cx<T>* __restrict__ tw, Ld ld) const {
    F::run_to_lds(lds, tw, ld);
  }
  __device__ __forceinline__ void lds_to_lds(cx<T>* lds, const cx<T>* __restrict__ tw) const {
    F::run_to_lds(lds, tw, NoLoad{});
  }
  template <class Ld, class St>
  __device__ __forceinline__ void global_to_global(cx<T>* lds, const cx<T>* __restrict__ tw, Ld ld, St st) const {
    F::run(lds, tw, ld, st);
  }
  // host side
  static int h_lines() { return F::B; }
  static int h_threads() { return F::NT; }
  static std::size_t h_lds() { return F::lds_bytes(); }
};
template <typename T, int N, int S, bool LF = false, bool TwPre = true>
struct CtEng : CtEngS<T, N, S, LF, TwPre, S> {};

// Run-time length engine. LF (line-fast) engines walk the global side with the
// line index fastest — consecutive lanes touch consecutive lines, i.e. the
// contiguous z-run of a stick or y-run of an intermediate column — like the
// compile-time line-fast mapping; row engines walk positions fastest.
template <typename T, int S, bool LF = false>
struct RtEng {
  static constexpr bool kBatchedCopy = true;
  static constexpr bool kLineFast = LF;
  static constexpr int kBlock = kRtThreads;
  RtPlan p;
  __device__ __forceinline__ int lines() const { return p.lines; }
  __device__ __forceinline__ int n() const { return p.n; }
  __device__ __forceinline__ int in_at(int b, int pos) const { return b * p.ls + pos; }
  __device__ __forceinline__ int out_at(int b, int pos) const {
    return ((!p.inplace && (p.np & 1)) ? p.lines * p.ls : 0) + b * p.ls + pos;
  }
  __device__ __forceinline__ int input_elems() const { return p.lines * p.ls; }
  __device__ __forceinline__ int lds_bytes() const {
    return (p.inplace ? 1 : 2) * p.lines * p.ls * static_cast<int>(sizeof(cx<T>));
  }
  // global-side element idx -> (line b, position pos); plan lines are a power
  // of two (make_rt_plan), so the line-fast split is a mask and a shift, and
  // the row split divides by a precomputed reciprocal
  __device__ __forceinline__ void split(int idx, int& b, int& pos) const {
    if (LF) {
      b = idx & (p.lines - 1);
      pos = idx >> p.linesLog2;
    } else {
      b = p.n == 1 ? idx : static_cast<int>(__umulhi(static_cast<unsigned>(idx), p.nMagic));
      pos = idx - b * p.n;
    }
  }
  template <class St>
  __device__ __forceinline__ void lds_to_global(cx<T>* lds, const cx<T>* __restrict__ tw, St st) const {
    const cx<T>* res = FftRT<T, S>::run_in_lds(p, lds, tw);
    store_from(res, st);
  }
  // input -> LDS at in_at(b, pos), no barrier (kernels with several input
  // paths stage each and then run the FFT once: one inlined copy of the passes)
  template <class Ld>
  __device__ __forceinline__ void stage(cx<T>* lds, Ld ld) const {
    gather_to_lds(lds, p.lines * p.n, [&](int idx) {
      int b, pos;
      split(idx, b, pos);
      return ld(b, pos);
    }, [&](int idx) {
      int b, pos;
      split(idx, b, pos);
      return b * p.ls + pos;
    });
  }
  template <class Ld>
  __device__ __forceinline__ void global_to_lds(cx<T>* lds, const cx<T>* __restrict__ tw, Ld ld) const {
    stage(lds, ld);
    __syncthreads();
    FftRT<T, S>::run_in_lds(p, lds, tw);
  }
  __device__ __forceinline__ void lds_to_lds(cx<T>* lds, const cx<T>* __restrict__ tw) const {
    FftRT<T, S>::run_in_lds(p, lds, tw);
  }
  template <class Ld, class St>
  __device__ __forceinline__ void global_to_global(cx<T>* lds, const cx<T>* __restrict__ tw, Ld ld, St st) const {
    global_to_lds(lds, tw, ld);
    store_from(lds + out_at(0, 0), st);
  }
  // result region res (index b * ls + pos) -> st(b, pos, v)
  template <class St>
  __device__ __forceinline__ void store_from(const cx<T>* res, St st) const {
    scatter_from_lds(res, p.lines * p.n, [&](int idx) {
      int b, pos;
      split(idx, b, pos);
      return b * p.ls + pos;
    }, [&](int idx, cx<T> v) {
      int b, pos;
      split(idx, b, pos);
      st(b, pos, v);
    });
  }
};

// Bluestein engine for lengths with a large prime factor (chirp-z: one
// convolution of power-of-two length m >= 2n-1 done with two run-time FFTs in
// LDS). X_k = d_k sum_j (x_j d_j) conj(d_{k-j}), d_j = exp(S i pi j^2 / n).
// Tables (device, per length): chirp d (S = -1) [n], FFT_m of the conj(d)
// filter for S = -1 and S = +1 [2m], twiddles of length m [m].
template <typename T, int S>
struct BlueEng {
  static constexpr bool kBatchedCopy = true;
  static constexpr bool kLineFast = false;
  static constexpr int kBlock = kMaxThreads;
  RtPlan pm;  // length m, ls = m
  int nn;
  const cx<T>* chirp;
  const cx<T>* filt;
  const cx<T>* twm;
  __device__ __forceinline__ int lines() const { return pm.lines; }
  __device__ __forceinline__ int n() const { return nn; }
  __device__ __forceinline__ int in_at(int b, int pos) const { return b * pm.ls + pos; }
  __device__ __forceinline__ int out_at(int b, int pos) const { return b * pm.ls + pos; }
  __device__ __forceinline__ int input_elems() const { return pm.lines * pm.ls; }
  __device__ __forceinline__ int lds_bytes() const { return 2 * pm.lines * pm.ls * static_cast<int>(sizeof(cx<T>)); }
  __device__ __forceinline__ cx<T> d(int j) const { return S < 0 ? chirp[j] : conj(chirp[j]); }
  __device__ __forceinline__ void run(cx<T>* lds) const {
    const int m = pm.n, total = pm.lines * m;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int b = idx / m, j = idx - b * m;
      cx<T>& v = lds[b * pm.ls + j];
      v = j < nn ? cmul(v, d(j)) : mk<T>(T(0), T(0));
    }
    __syncthreads();
    cx<T>* A = lds;
    cx<T>* B = lds + pm.lines * pm.ls;
    cx<T>* r = FftRT<T, -1>::run_between(pm, A, B, twm);
    const cx<T>* f = filt + (S < 0 ? 0 : m);
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int b = idx / m, j = idx - b * m;
      r[b * pm.ls + j] = cmul(r[b * pm.ls + j], f[j]);
    }
    __syncthreads();
    cx<T>* r2 = FftRT<T, +1>::run_between(pm, r, r == A ? B : A, twm);
    const T inv = T(1) / static_cast<T>(m);
    for (int idx = threadIdx.x; idx < pm.lines * nn; idx += blockDim.x) {
      const int b = idx / nn, k = idx - b * nn;
      A[b * pm.ls + k] = scale(cmul(r2[b * pm.ls + k], d(k)), inv);
    }
    __syncthreads();
  }
  template <class St>
  __device__ __forceinline__ void lds_to_global(cx<T>* lds, const cx<T>* __restrict__, St st) const {
    run(lds);
    store_from(lds, st);
  }
  template <class Ld>
  __device__ __forceinline__ void stage(cx<T>* lds, Ld ld) const {
    gather_to_lds(lds, pm.lines * nn, [&](int idx) {
      const int b = idx / nn;
      return ld(b, idx - b * nn);
    }, [&](int idx) {
      const int b = idx / nn;
      return in_at(b, idx - b * nn);
    });
  }
  template <class Ld>
  __device__ __forceinline__ void global_to_lds(cx<T>* lds, const cx<T>* __restrict__, Ld ld) const {
    stage(lds, ld);
    __syncthreads();
    run(lds);
  }
  __device__ __forceinline__ void lds_to_lds(cx<T>* lds, const cx<T>* __restrict__) const { run(lds); }
  template <class Ld, class St>
  __device__ __forceinline__ void global_to_global(cx<T>* lds, const cx<T>* __restrict__ tw, Ld ld, St st) const {
    global_to_lds(lds, tw, ld);
    store_from(lds, st);
  }
  template <class St>
  __device__ __forceinline__ void store_from(const cx<T>* lds, St st) const {
    scatter_from_lds(lds, pm.lines * nn, [&](int idx) {
      const int b = idx / nn;
      return out_at(b, idx - b * nn);
    }, [&](int idx, cx<T> v) {
      const int b = idx / nn;
      st(b, idx - b * nn, v);
    });
  }
};

template <typename To, typename From>
__device__ __forceinline__ cx<To> cvt(const cx<From>& v) {
  return mk<To>(static_cast<To>(v.x), static_cast<To>(v.y));
}
template <typename T>
__device__ __forceinline__ bool nonzero(const cx<T>& v) {
  return v.x != T(0) || v.y != T(0);
}
template <typename T>
__device__ __forceinline__ cx<T> czero() {
  return mk<T>(T(0), T(0));
}

// Hermitian completion (only where the source is non-zero) of `count` LDS lines
// starting at line b0, with the two half passes of the reference
// (src/symmetry/gpu_kernels/symmetry_kernels.cu:56-78, 119-141) as two
// barrier-separated phases of one workgroup.
template <class Eng, typename T>
__device__ __forceinline__ void hermitian_lines_inline(const Eng& eng, cx<T>* lds, int b0, int count, int n) {
  const int h1 = n / 2;          // k in [1, n/2]
  const int h2 = n - 1 - h1;     // k in [n/2+1, n-1]
  for (int idx = threadIdx.x; idx < count * h1; idx += blockDim.x) {
    const int b = b0 + idx / h1, k = 1 + idx % h1;
    const cx<T> v = lds[eng.in_at(b, k)];
    if (nonzero(v)) lds[eng.in_at(b, n - k)] = conj(v);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < count * h2; idx += blockDim.x) {
    const int b = b0 + idx / h2, k = h1 + 1 + idx % h2;
    const cx<T> v = lds[eng.in_at(b, k)];
    if (nonzero(v)) lds[eng.in_at(b, n - k)] = conj(v);
  }
  __syncthreads();
}

// Out of line where the compiler decides so (the stage kernels); the fused
// reciprocal z stage inlines the body: a call would pass its engine, a run-time
// plan, through scratch memory.
template <class Eng, typename T>
__device__ void hermitian_lines(const Eng& eng, cx<T>* lds, int b0, int count, int n) {
  hermitian_lines_inline(eng, lds, b0, count, n);
}

template <typename T>
__device__ __forceinline__ void zero_lds(cx<T>* lds, int count) {
  for (int i = threadIdx.x; i < count; i += blockDim.x) lds[i] = czero<T>();
}

// A workgroup-uniform value materialised in a scalar register at this point:
// the compiler may not sink its (scalar) load into later branches.
__device__ __forceinline__ int pin_uniform(int v) {
  v = __builtin_amdgcn_readfirstlane(v);
  asm volatile("" : "+s"(v));
  return v;
}

__device__ __forceinline__ long long pin_uniform64(long long v) {
  int lo = pin_uniform(static_cast<int>(v)), hi = pin_uniform(static_cast<int>(v >> 32));
  return (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo);
}

// Exchange-side element of (stick s, plane pos): the plain stick array of a
// single rank, else the plane's segment (one 16-byte table entry per plane:
// no dependent loads). The arguments are pinned in scalar registers once per
// kernel (read through ZArgs per element, their scalar loads were sunk into
// every element's branch and waited out there).
struct SegMap {
  int single;
  long long stride;
  const long long* tab;
  __device__ explicit SegMap(const ZArgs& a)
      : single(pin_uniform(a.single)), stride(pin_uniform64(a.stickStride)), tab(a.zTab) {}
  __device__ long long at(int s, int pos) const {
    if (single == 1) return static_cast<long long>(s) * stride + pos;
    using V = long long __attribute__((ext_vector_type(2)));
    const V t = *reinterpret_cast<const V*>(tab + 2 * pos);
    return t.x + static_cast<long long>(s) * t.y;
  }
};

__device__ __forceinline__ long long seg_index(const ZArgs& a, int s, int pos) {
  return SegMap(a).at(s, pos);
}

#define SPFFT_LDS_DECL(T)                                         \
  extern __shared__ __attribute__((aligned(16))) char spfftSmem[]; \
  cx<T>* lds = reinterpret_cast<cx<T>*>(spfftSmem)

// Row side of a line-fast kernel: lanes walk along rows (row-contiguous global
// loads) into the FFT lines in LDS; line-fast lanes would touch B rows with
// (64/B)-element segments per wave instruction (32 B segments for fp32 B=16).
// Row b of the tile starts at base + b * stride: complex elements, or real ones
// (E == T) loaded with a zero imaginary part.
template <typename E>
struct RowSrc {
  const E* base;
  long long stride;
};
template <typename T, typename E>
__device__ __forceinline__ cx<T> row_elem(const E* p) {
  if constexpr (std::is_same<E, T>::value)
    return mk<T>(ld_stream_real(p), T(0));
  else
    return ld_stream(p);
}
// Pair row source (x_forward_pair_kernel): the element staged is conj(a) * b of
// two arrays with one row layout. PairPtr stands in for RowSrc's element
// pointer; Stream: the cache policy of both loads (non-temporal or plain).
template <typename T, bool Stream>
struct PairPtr {
  const cx<T>* a;
  const cx<T>* b;
  __device__ __forceinline__ PairPtr operator+(long long d) const { return PairPtr{a + d, b + d}; }
};
template <typename T, bool Stream>
struct PairSrc {
  PairPtr<T, Stream> base;
  long long stride;
};
template <typename T, bool Stream>
__device__ __forceinline__ cx<T> row_elem(PairPtr<T, Stream> p) {
  if constexpr (Stream) return cmulc(ld_stream(p.b), ld_stream(p.a));
  else return cmulc(*p.b, *p.a);
}
// Packed-real pair row source (x_forward_pair_r2c_kernel): a and b are real
// arrays read as pairs (s[2m], s[2m+1]), and the element staged is the packed
// row of their product, a[2m] b[2m] + i a[2m+1] b[2m+1]: a component-wise
// product, not a complex one (conj is the identity for real fields). Both
// pointers must be aligned to one pair.
template <typename T, bool Stream>
struct PairRealPtr {
  const cx<T>* a;
  const cx<T>* b;
  __device__ __forceinline__ PairRealPtr operator+(long long d) const { return PairRealPtr{a + d, b + d}; }
};
template <typename T, bool Stream>
struct PairRealSrc {
  PairRealPtr<T, Stream> base;
  long long stride;
};
template <typename T, bool Stream>
__device__ __forceinline__ cx<T> row_elem(PairRealPtr<T, Stream> p) {
  cx<T> x, y;
  if constexpr (Stream) {
    x = ld_stream(p.a);
    y = ld_stream(p.b);
  } else {
    x = *p.a;
    y = *p.b;
  }
  return mk<T>(x.x * y.x, x.y * y.y);
}
// Src: RowSrc<E>, PairSrc<T, Stream> or PairRealSrc<T, Stream>
template <class Eng, typename T, class Src>
__device__ __forceinline__ void stage_rows(const Eng& eng, cx<T>* lds, int rows, int len, Src src) {
  if constexpr (!Eng::kBatchedCopy) {
    // full tile of a compile-time engine: the trip count, and each unrolled
    // load's row and position offsets, are compile-time (the row products are
    // scalar), so the generic loop's per-element guards, divisions and 64-bit
    // row multiplies go (fp32 y forward: 3 quarter-rate multiplies per load)
    using F = typename Eng::F;
    constexpr int N = Eng::kN, NT = F::NT, B = F::B;
    constexpr int kIters = B * N / NT;
    // (not the wide 512-thread engines: their kernels sit at the 128-VGPR
    // occupancy step, fp32 512 y forward 127 -> 131 VGPRs and 241 -> 316 us with it)
    if constexpr ((B * N) % NT == 0 && (NT % N == 0 || N % NT == 0) && kIters <= 32 &&
                  NT <= kMaxThreads) {
      if (rows == B) {
        const int tid = static_cast<int>(threadIdx.x);
        cx<T> v[kIters];
        if constexpr (NT % N == 0) {
          constexpr int RP = NT / N;  // rows per pass of the workgroup
          const int b0 = tid / N, p = tid % N;
          const auto p0 = src.base + static_cast<long long>(b0) * src.stride + p;
#pragma unroll
          for (int i = 0; i < kIters; ++i) v[i] = row_elem<T>(p0 + (i * RP) * src.stride);
#pragma unroll
          for (int i = 0; i < kIters; ++i) lds[eng.in_at(b0 + i * RP, p)] = v[i];
        } else {
          constexpr int C = N / NT;  // passes per row
          const auto p0 = src.base + tid;
#pragma unroll
          for (int i = 0; i < kIters; ++i) v[i] = row_elem<T>(p0 + (i / C) * src.stride + (i % C) * NT);
#pragma unroll
          for (int i = 0; i < kIters; ++i) lds[eng.in_at(i / C, tid + (i % C) * NT)] = v[i];
        }
        __syncthreads();
        return;
      }
    }
  }
  gather_to_lds(lds, rows * len, [&](int idx) {
    const int b = idx / len;
    if (b >= rows) return czero<T>();
    return row_elem<T>(src.base + static_cast<long long>(b) * src.stride + (idx - b * len));
  }, [&](int idx) {
    const int b = idx / len;
    return eng.in_at(b, idx - b * len);
  });
  __syncthreads();
}

// Exclusive prefix sum of n ints in LDS (one wave, 64-wide shuffle scans); writes
// out[0..n] (out[n] = total). Ends with a barrier.
__device__ __forceinline__ void wave_exclusive_scan(const int* in, int* out, int n) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int c = 0; c < n; c += 64) {
      const int i = c + lane;
      const int v = i < n ? in[i] : 0;
      int x = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
      }
      if (i < n) out[i] = carry + x - v;
      carry += __shfl(x, 63, 64);
    }
    if (lane == 0) out[n] = carry;
  }
  __syncthreads();
}

// Run table of a block of sticks staged in LDS (after the FFT lines):
// the gather/scatter between sparse values and sticks is then one flat loop
// with all loads independent (value index = first + idx when the block's runs
// are consecutive in value order, the common stick-major input).
struct RunTable {
  StickRun* runs;
  int* start;  // exclusive prefix of run lengths, count+1 entries
  int count;
  int total;
  bool contiguous;
};

constexpr int kRunsPerLine = 4;  // table capacity per stick line

__host__ __device__ constexpr std::size_t run_table_bytes(int lines) {
  return std::size_t(kRunsPerLine) * lines * (sizeof(StickRun) + sizeof(int)) + 16 >
                 std::size_t(lines) * sizeof(StickDesc)
             ? std::size_t(kRunsPerLine) * lines * (sizeof(StickRun) + sizeof(int)) + 16
             : std::size_t(lines) * sizeof(StickDesc);
}

// Returns false if the block's runs do not fit the table (caller falls back).
__device__ __forceinline__ bool load_run_table(const ZArgs& a, int s0, int lines, char* base,
                                               RunTable& t) {
  const int s1 = min(s0 + lines, a.numSticks);
  const int q0 = a.runOffsets[s0];
  const int q1 = a.runOffsets[s1];
  const int R = q1 - q0;
  if (R > kRunsPerLine * lines) return false;  // block-uniform
  t.runs = reinterpret_cast<StickRun*>(base);
  int* lens = reinterpret_cast<int*>(base + sizeof(StickRun) * kRunsPerLine * lines);
  t.start = lens;  // scanned in place into a shifted copy below
  int ok = 1;
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    const StickRun r = a.runs[q0 + i];
    t.runs[i] = r;
    if (i > 0) {
      const StickRun p = a.runs[q0 + i - 1];
      if (p.valueStart + p.length != r.valueStart) ok = 0;
    }
  }
  t.contiguous = __syncthreads_and(ok) != 0;
  // prefix of lengths (wave 0), lengths read from the staged runs
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int c = 0; c < R; c += 64) {
      const int i = c + lane;
      const int v = i < R ? t.runs[i].length : 0;
      int x = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
      }
      if (i < R) lens[i] = carry + x - v;
      carry += __shfl(x, 63, 64);
    }
    if (lane == 0) lens[R] = carry;
  }
  __syncthreads();
  t.count = R;
  t.total = lens[R];
  return true;
}

// index of the run containing flat element idx (binary search over start[])
__device__ __forceinline__ int find_run(const RunTable& t, int idx) {
  int lo = 0, hi = t.count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.start[mid] <= idx)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// Exchange-side addressing of the z stage kernels. A single rank's stick array
// is pure arithmetic (stride pinned in scalar registers). Distributed plans
// stage their per-plane segment table, (base, stride) per plane z (ZArgs::zTab),
// in LDS once per workgroup: read from global memory per element, a table
// entry's wait (s_waitcnt vmcnt) also waited out every data load the lane had
// issued before it, while LDS reads count separately (lgkmcnt). Only
// distributed launches reserve the table's LDS: at 256^3 fp64 its 4 KB cost
// the z forward kernel a third of its workgroups per CU (66 -> 73 us), as did
// computing a single rank's table in LDS. (A kernel template per plan kind
// doubled the z kernels and tripled their compile time.)
// Distributed launches whose engine leaves no room for the table (long z lines
// near the LDS limit) read it from global memory instead (ZArgs::single = 2,
// set by the launcher: z_args_for_lds).
struct ZSeg {
  int single;
  long long stride;
  const long long* tab;   // LDS (distributed plans)
  const long long* gtab;  // global memory (single == 2)
  __device__ ZSeg(const ZArgs& a, char* ldsTab, int n)
      : single(pin_uniform(a.single)), stride(pin_uniform64(a.stickStride)),
        tab(reinterpret_cast<const long long*>(ldsTab)), gtab(a.zTab) {
    if (single == 0) {
      long long* t = reinterpret_cast<long long*>(ldsTab);
      for (int i = threadIdx.x; i < 2 * n; i += blockDim.x) t[i] = a.zTab[i];
      __syncthreads();
    }
  }
  // the same from the fields alone, always inlined (a call would pass ZArgs
  // through scratch memory: the fused reciprocal z stage)
  __device__ __forceinline__ ZSeg(int single_, long long stride_, const long long* zTab, char* ldsTab, int n)
      : single(pin_uniform(single_)), stride(pin_uniform64(stride_)),
        tab(reinterpret_cast<const long long*>(ldsTab)), gtab(zTab) {
    if (single == 0) {
      long long* t = reinterpret_cast<long long*>(ldsTab);
      for (int i = threadIdx.x; i < 2 * n; i += blockDim.x) t[i] = zTab[i];
      __syncthreads();
    }
  }
  __device__ long long at(int s, int pos) const {
    using V = long long __attribute__((ext_vector_type(2)));
    if (single == 1) return static_cast<long long>(s) * stride + pos;
    if (single == 2) {
      const V t = *reinterpret_cast<const V*>(gtab + 2 * pos);
      return t.x + static_cast<long long>(s) * t.y;
    }
    const V t = *reinterpret_cast<const V*>(tab + 2 * pos);
    return t.x + static_cast<long long>(s) * t.y;
  }
};
// LDS offset of ZSeg's table behind the FFT lines and the desc / run table
__host__ __device__ constexpr std::size_t zseg_lds_offset(std::size_t fftBytes, int lines) {
  return (fftBytes + run_table_bytes(lines) + 15) / 16 * 16;
}
inline std::size_t zseg_lds_bytes(const ZArgs& a) {
  return a.single ? 0 : std::size_t(2) * a.n * sizeof(long long) + 16;
}
// The launch's arguments and LDS bytes: a distributed plan's segment table
// moves to global memory when it would push the workgroup past the LDS limit.
inline ZArgs z_args_for_lds(const ZArgs& a, std::size_t fftBytes, int lines, std::size_t* ldsTotal) {
  ZArgs b = a;
  constexpr std::size_t kLimit = 160 * 1024;
  if (!b.single && zseg_lds_offset(fftBytes, lines) + zseg_lds_bytes(b) > kLimit) b.single = 2;
  *ldsTotal = zseg_lds_offset(fftBytes, lines) + zseg_lds_bytes(b);
  return b;
}

// Workgroup -> tile mapping: the dispatcher deals consecutive workgroups
// round-robin to the 8 XCDs. An XCD-contiguous remap was measured slower on
// MI355X at 256^3 (x/y stages 3-6 us, bench -4.5%, profiles/r2_s1/shape_ab.txt):
// the stages have no cross-workgroup reuse for an XCD's L2, and round-robin
// spreads the addresses in flight over all eight XCDs' paths to HBM.
__device__ __forceinline__ void block_tile(int& bx, int& by) {
  bx = blockIdx.x;
  by = blockIdx.y;
}
__device__ __forceinline__ int block_tile_x() { return blockIdx.x; }

// Batched launch (ZArgs/YArgs/XArgs::batch): the workgroup's transform
// (blockIdx.z) supplies the input and output buffers; the index tables are
// shared by every transform of the batch.
#define SPFFT_BATCH_SELECT(a, IN, OUT)                                   \
  if ((a).batch.count > 1) {                                           \
    IN = static_cast<decltype(IN)>((a).batch.in[blockIdx.z]);          \
    OUT = static_cast<decltype(OUT)>((a).batch.out[blockIdx.z]);       \
  }

// ---------------------------------------------------------------- z stage
template <class Eng, typename T, typename BT>
__global__ void __launch_bounds__(Eng::kBlock)
    z_backward_kernel(Eng eng, ZArgs a, const cx<T>* __restrict__ values, BT* __restrict__ out,
                      const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, values, out);
  const int B = eng.lines();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const ZSeg seg(a, reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), eng.n());
  zero_lds(lds, eng.input_elems());
  RunTable tab;
  char* tableBase = reinterpret_cast<char*>(lds) + eng.lds_bytes();
  if (load_run_table(a, s0, B, tableBase, tab)) {
    // decompress: flat over the block's values, kGatherUnroll loads in flight per lane
    if (tab.contiguous) {
      const cx<T>* src = values + tab.runs[0].valueStart;
      gather_to_lds(lds, tab.total, [&](int idx) { return src[idx]; }, [&](int idx) {
        const int q = find_run(tab, idx);
        return eng.in_at(tab.runs[q].stick - s0, tab.runs[q].zStart + idx - tab.start[q]);
      });
    } else {
      gather_to_lds(lds, tab.total, [&](int idx) {
        const int q = find_run(tab, idx);
        return ld_values(&values[tab.runs[q].valueStart + idx - tab.start[q]]);
      }, [&](int idx) {
        const int q = find_run(tab, idx);
        return eng.in_at(tab.runs[q].stick - s0, tab.runs[q].zStart + idx - tab.start[q]);
      });
    }
  } else {
    // many short runs (unsorted input): one wave per stick
    __syncthreads();  // zero-fill complete
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int b = wave; b < B; b += nw) {
      const int s = s0 + b;
      if (s >= a.numSticks) break;
      const int q1 = a.runOffsets[s + 1];
      for (int q = a.runOffsets[s]; q < q1; ++q) {
        const StickRun r = a.runs[q];
        for (int j = lane; j < r.length; j += 64)
          lds[eng.in_at(b, r.zStart + j)] = ld_values(&values[r.valueStart + j]);
      }
    }
  }
  __syncthreads();
  if (a.zeroStick >= s0 && a.zeroStick < s0 + B) hermitian_lines(eng, lds, a.zeroStick - s0, 1, a.n);
  eng.lds_to_global(lds, tw, [&](int b, int pos, cx<T> v) {
    const int s = s0 + b;
    if (s < a.numSticks) st_stream(&out[seg.at(s, pos)], cvt<typename BT::value_type>(v));
  });
}

template <class Eng, typename T, typename BT>
__global__ void __launch_bounds__(Eng::kBlock)
    z_forward_kernel(Eng eng, ZArgs a, const BT* __restrict__ in, cx<T>* __restrict__ values,
                     T scale, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, in, values);
  const int B = eng.lines();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const ZSeg seg(a, reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), eng.n());
  eng.global_to_lds(lds, tw, [&](int b, int pos) -> cx<T> {
    const int s = s0 + b;
    if (s >= a.numSticks) return czero<T>();
    return cvt<T>(ld_stream(&in[seg.at(s, pos)]));
  });
  // compress (+ scaling)
  RunTable tab;
  char* tableBase = reinterpret_cast<char*>(lds) + eng.lds_bytes();
  if (load_run_table(a, s0, B, tableBase, tab)) {
    for (int idx = threadIdx.x; idx < tab.total; idx += blockDim.x) {
      const int q = find_run(tab, idx);
      const StickRun& r = tab.runs[q];
      const int off = idx - tab.start[q];
      st_values(&values[r.valueStart + off], spfft::scale(lds[eng.out_at(r.stick - s0, r.zStart + off)], scale));
    }
  } else {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int b = wave; b < B; b += nw) {
      const int s = s0 + b;
      if (s >= a.numSticks) break;
      const int q1 = a.runOffsets[s + 1];
      for (int q = a.runOffsets[s]; q < q1; ++q) {
        const StickRun r = a.runs[q];
        for (int j = lane; j < r.length; j += 64)
          st_values(&values[r.valueStart + j], spfft::scale(lds[eng.out_at(b, r.zStart + j)], scale));
      }
    }
  }
}

// z stage for "simple" sticks (values of a stick contiguous, <= 2 z-runs; the
// common stick-major input): every lane maps its FFT positions z straight to
// value offsets, so values are loaded into registers and written back with
// coalesced accesses and no LDS staging or zero-fill.
__device__ __forceinline__ int desc_offset(const StickDesc& q, int z) {
  int j = z - q.z0;
  if (j >= 0 && j < q.len0) return j;
  j = z - q.z1;
  if (j >= 0 && j < q.count - q.len0) return q.len0 + j;
  return -1;
}

template <class Eng, typename T, typename BT, bool Plain>
__global__ void __launch_bounds__(Eng::kBlock)
    z_backward_desc_kernel(Eng eng, ZArgs a, const cx<T>* __restrict__ values,
                           BT* __restrict__ out, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, values, out);
  const int B = eng.lines();
  const int n = eng.n();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const int nl = min(B, a.numSticks - s0);
  const ZSeg seg(a, reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), eng.n());
  auto store = [&](int b, int pos, cx<T> v) {
    if (b < nl) st_stick<Plain>(&out[seg.at(s0 + b, pos)], cvt<typename BT::value_type>(v));
  };
  StickDesc* d = reinterpret_cast<StickDesc*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  for (int b = threadIdx.x; b < nl; b += blockDim.x) d[b] = a.desc[s0 + b];
  __syncthreads();
  auto load = [&](int b, int z) -> cx<T> {
    if (b >= nl) return czero<T>();
    const StickDesc& q = d[b];
    const int j = desc_offset(q, z);
    return j < 0 ? czero<T>() : ld_values(&values[q.valueStart + j]);
  };
  if constexpr (Eng::kBatchedCopy) {
    // run-time engines: one staged path for every block (a single inlined copy
    // of the pass switch keeps the kernel's register demand down)
    eng.stage(lds, load);
    __syncthreads();
    if (a.zeroStick >= s0 && a.zeroStick < s0 + nl) hermitian_lines(eng, lds, a.zeroStick - s0, 1, n);
    eng.lds_to_global(lds, tw, store);
  } else if (a.zeroStick >= s0 && a.zeroStick < s0 + nl) {
    // block holding the (0,0) stick of an R2C transform: stage for the hermitian fill
    for (int idx = threadIdx.x; idx < B * n; idx += blockDim.x) {
      const int b = idx / n, z = idx - b * n;
      lds[eng.in_at(b, z)] = load(b, z);
    }
    __syncthreads();
    hermitian_lines(eng, lds, a.zeroStick - s0, 1, n);
    eng.lds_to_global(lds, tw, store);
  } else {
    // compile-time engines load only the lane's own line (b == lane_line(),
    // the FftCT/FftMR contract): its descriptor is read from LDS once into
    // registers and the value offset is a branch-free select. Reading d[b] in
    // the load lambda re-read the descriptor from LDS for every element, each
    // read waited out before the dependent value load could issue.
    const int lb = Eng::F::lane_line();
    StickDesc q = d[lb < nl ? lb : 0];
    int z0 = q.z0, len0 = q.len0, z1 = q.z1, len1 = q.count - q.len0, vs = q.valueStart;
    if (lb >= nl) len0 = len1 = 0;
    asm volatile("" : "+v"(z0), "+v"(len0), "+v"(z1), "+v"(len1), "+v"(vs));
    const cx<T>* vals = values + vs;
    eng.global_to_global(lds, tw, [&](int, int z) -> cx<T> {
      const unsigned j0 = static_cast<unsigned>(z - z0), j1 = static_cast<unsigned>(z - z1);
      const bool in0 = j0 < static_cast<unsigned>(len0);
      const bool in1 = j1 < static_cast<unsigned>(len1);
      const int j = in0 ? static_cast<int>(j0) : len0 + static_cast<int>(j1);
      // streamed value loads: 256^3 fp64 79.2 -> 63.4 us, 512^3 R2C fp32 219 ->
      // 133 us, fp32 256^3 neutral (T = 1, same box; profiles/r6/ntmerge)
      return (in0 || in1) ? ld_stream(&vals[j]) : czero<T>();
    }, store);
  }
}

template <class Eng, typename T, typename BT, bool NtValues>
__global__ void __launch_bounds__(Eng::kBlock)
    z_forward_desc_kernel(Eng eng, ZArgs a, const BT* __restrict__ in, cx<T>* __restrict__ values,
                          T scale, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, in, values);
  const int B = eng.lines();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const int nl = min(B, a.numSticks - s0);
  const ZSeg seg(a, reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), eng.n());
  if constexpr (!Eng::kBatchedCopy) {
    // compile-time engines: the lane's own stick descriptor in registers, no
    // LDS round trip (69.6 -> 65.0 us at 256^3, profiles/r1_s14/zdesc_ab/
    // summary.txt; the same change in the backward kernel, whose value loads
    // are on the critical path, measured 81 -> 104 us). This relies on the
    // compile-time engines' run() storing only the lane's own line
    // (b == lane_line()); the assert guards that contract in debug builds.
    const int lb = Eng::F::lane_line();
    StickDesc q{};
    if (lb < nl) q = a.desc[s0 + lb];
    const int z0 = q.z0, len0 = lb < nl ? q.len0 : 0, z1 = q.z1, len1 = lb < nl ? q.count - q.len0 : 0;
    cx<T>* vals = values + q.valueStart;
    auto store = [&](int b, int pos, cx<T> v) {
      assert(b == lb);
      // branch-free value offset (as in the backward kernel); one predicated store
      const unsigned j0 = static_cast<unsigned>(pos - z0), j1 = static_cast<unsigned>(pos - z1);
      const bool in0 = j0 < static_cast<unsigned>(len0);
      const bool in1 = j1 < static_cast<unsigned>(len1);
      const int j = in0 ? static_cast<int>(j0) : len0 + static_cast<int>(j1);
      if (in0 || in1) {
        if constexpr (NtValues) st_stream(&vals[j], spfft::scale(v, scale));
        else st_values(&vals[j], spfft::scale(v, scale));
      }
    };
    // Lanes past the last stick load a valid stick (min(lb, nl - 1)) and store
    // nothing (len0 = len1 = 0): no guard per element. Loads only the lane's own
    // line (b == lb, the FftCT/FftMR contract).
    const int ls = s0 + min(lb, nl - 1);
    if (seg.single == 1) {
      // plain stick rows (one rank): the row is the lane's base pointer, each
      // element a constant offset from it; no segment-mode branch and no 64-bit
      // multiply per element (the other modes below read a table per position)
      const BT* row = in + static_cast<long long>(ls) * seg.stride + Eng::F::lane_pos();
      eng.global_to_global(lds, tw, [&](int, int, int off) -> cx<T> { return cvt<T>(ld_stream(&row[off])); },
                           store);
    } else {
      eng.global_to_global(lds, tw, [&](int, int pos) -> cx<T> {
        return cvt<T>(ld_stream(&in[seg.at(ls, pos)]));
      }, store);
    }
  } else {
    StickDesc* d = reinterpret_cast<StickDesc*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
    for (int b = threadIdx.x; b < nl; b += blockDim.x) d[b] = a.desc[s0 + b];
    __syncthreads();
    eng.global_to_global(lds, tw, [&](int b, int pos) -> cx<T> {
      if (b >= nl) return czero<T>();
      return cvt<T>(ld_stream(&in[seg.at(s0 + b, pos)]));
    }, [&](int b, int pos, cx<T> v) {
      if (b >= nl) return;
      const StickDesc& q = d[b];
      const int j = desc_offset(q, pos);
      if (j >= 0) {
        if constexpr (NtValues) st_stream(&values[q.valueStart + j], spfft::scale(v, scale));
        else st_values(&values[q.valueStart + j], spfft::scale(v, scale));
      }
    });
  }
}

// y-stage tile order: plane blocks fastest in the grid, so the workgroups in
// flight cover a few whole columns: each stick is read (or written) entirely
// while it is open in the DRAM row buffers, and the [z][column][y] rows of a
// plane are written as one contiguous run.
__device__ __forceinline__ int y_tile_col() {
  int bx, by;
  block_tile(bx, by);
  return by;
}
__device__ __forceinline__ int y_tile_zblock() {
  int bx, by;
  block_tile(bx, by);
  return bx;
}
inline dim3 y_grid(int cols, int zblocks, unsigned batch = 1) { return dim3(zblocks, cols, batch); }

// ---------------------------------------------------------------- y stage
// Whether the column with run descriptor d has a stick entry at y, and its base
// (uniform loop bound nRuns: a sphere column tests its 2 runs only).
__device__ __forceinline__ bool col_desc_find(const ColDesc& d, long long stride, int y,
                                              long long& base) {
  long long b0 = 0;
  bool hit = false;
#pragma unroll
  for (int r = 0; r < kColRuns; ++r) {
    if (r < d.nRuns) {
      const bool in = static_cast<unsigned>(y - d.y[r]) < static_cast<unsigned>(d.len[r]);
      b0 = in ? d.b0[r] : b0;
      hit = hit || in;
    }
  }
  base = b0 + static_cast<long long>(static_cast<unsigned>(y) * static_cast<unsigned>(stride));
  return hit;
}

// Stick entries of the workgroup's column: through the column's run descriptor
// (workgroup-uniform, scalar registers, no prologue) when the plan has one, else
// through the entry list staged in LDS (colBase per entry, y -> entry table).
// Every kernel keeps a single FFT call site whichever source is used: the
// run-time engines inline their whole pass switch per call site, and a second
// copy doubled their register demand (profiles/r2_s1/rt_regression.txt).
// engines whose store positions can be enumerated ahead of run() (FftCT)
template <class Eng, class = void>
struct has_store_pos : std::false_type {};
template <class Eng>
struct has_store_pos<Eng, std::void_t<decltype(Eng::F::kStoreSlots)>> : std::true_type {};
// "No stick entry" in the y -> base tables. Bases are element offsets from the
// stage's buffer, and the peer-write plane's are offsets to the peers' buffers,
// which lie below the local one as often as above: -1 would be a valid base.
constexpr long long kNoBase = -(1LL << 62);

template <class Eng>
struct ColEntries {
  bool useDesc;
  ColDesc d;
  long long stride;
  long long* yBase;  // LDS: y -> stick-side base or kNoBase (table mode)
  long long* cBase;  // LDS: colBase per entry (list mode)
  int* yEnt;         // LDS: y -> entry or -1 (list mode)
  int* cY;           // LDS: entry -> y (list mode)
  int ne;
  // table: build only yBase, the y -> base table (the backward y stage's loads
  // then cost one LDS read per element instead of a descriptor search per
  // element and lane); it shares its LDS with the list-mode arrays, which the
  // table mode does not use
  __device__ ColEntries(const Eng& eng, const YArgs& a, void* ldsBase, int c, bool allowDesc,
                        bool table = false) {
    const int n = eng.n();
    useDesc = allowDesc && a.colDesc != nullptr;
    stride = a.colStride;
    char* base = reinterpret_cast<char*>(ldsBase) + eng.lds_bytes();
    yBase = reinterpret_cast<long long*>(base);
    cBase = yBase;
    yEnt = reinterpret_cast<int*>(cBase + n);
    cY = yEnt + n;
    ne = 0;
    if (useDesc) {
      d = a.colDesc[c];
      if (table) {
        for (int y = threadIdx.x; y < n; y += blockDim.x) {
          long long b;
          yBase[y] = col_desc_find(d, stride, y, b) ? b : kNoBase;
        }
        __syncthreads();
      }
      return;
    }
    const int k0 = a.colOffsets[c];
    ne = a.colOffsets[c + 1] - k0;
    if (table) {
      for (int y = threadIdx.x; y < n; y += blockDim.x) yBase[y] = kNoBase;
      __syncthreads();
      for (int e = threadIdx.x; e < ne; e += blockDim.x) yBase[a.colY[k0 + e]] = a.colBase[k0 + e];
      __syncthreads();
      return;
    }
    for (int y = threadIdx.x; y < n; y += blockDim.x) yEnt[y] = -1;
    __syncthreads();
    for (int e = threadIdx.x; e < ne; e += blockDim.x) {
      const int y = a.colY[k0 + e];
      cBase[e] = a.colBase[k0 + e];
      yEnt[y] = e;
      cY[e] = y;
    }
    __syncthreads();
  }
  // whether the column has an entry at y; its base (add the plane) in base
  __device__ bool find(int y, long long& base) const {
    if (useDesc) return col_desc_find(d, stride, y, base);
    const int e = yEnt[y];
    base = e < 0 ? 0 : cBase[e];
    return e >= 0;
  }
};

// LDS the y-stage kernels reserve behind the FFT lines for ColEntries: the list
// mode (colBase, y -> entry, entry -> y) where it can run, and the y -> base
// table (table: the kernel runs table mode; both share one region). With column
// run descriptors only the backward R2C x = 0 column (hermitian fill) runs list
// mode; C2C forward plans reserve nothing, which keeps fp32 N = 256 at 4
// workgroups per CU.
inline std::size_t col_entries_lds(const YArgs& a, bool backward, bool table = false) {
  const bool list = !a.colDesc || (backward && a.colOfX0 >= 0);
  std::size_t bytes = list ? std::size_t(a.n) * (sizeof(long long) + 2 * sizeof(int)) : 0;
  if (table) bytes = std::max(bytes, std::size_t(a.n) * sizeof(long long));
  return bytes ? bytes + 16 : 0;
}

constexpr std::size_t kLdsPerWorkgroup = 160 * 1024;

// Whether a y-stage kernel with engine Eng runs table mode: compile-time
// engines (one LDS read per element replaces their per-element search) whose
// FFT lines leave room for the table next to the list-mode arrays.
template <class Eng, bool Enabled>
constexpr bool y_table() {
  if constexpr (Eng::kBatchedCopy || !Enabled) {
    return false;
  } else {
    constexpr int n = Eng::kN;
    return Eng::F::lds_bytes() + std::size_t(n) * (sizeof(long long) + 2 * sizeof(int)) + 16 <=
           kLdsPerWorkgroup;
  }
}

// Backward y stage with the line-fast engine: lane (line = plane zz, pos = y)
// loads straight from the stick side — consecutive lanes read consecutive z
// of one stick (coalesced) — with no LDS staging of the input. The x = 0
// column of an R2C transform is gathered into LDS for the hermitian fill.
template <class Eng, typename T, typename BT, bool Plain>
__global__ void __launch_bounds__(Eng::kBlock)
    y_backward_kernel(Eng eng, YArgs a, const BT* __restrict__ in, cx<T>* __restrict__ inter,
                      const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, in, inter);
  const int B = eng.lines();
  const int n = eng.n();
  const int c = a.colBegin + y_tile_col();
  const int z0 = a.zBegin + y_tile_zblock() * B;
  const int zl = min(B, a.L - z0);
  const bool x0 = c == a.colOfX0;
  constexpr bool kTable = y_table<Eng, true>();
  const ColEntries<Eng> ce(eng, a, lds, c, !x0, kTable && !x0);
  auto load = [&](int b, int pos) -> cx<T> {
    if constexpr (kTable) {
      const long long base = ce.yBase[pos];
      // masked load: the lanes of a missing stick issue no request at all (a shared
      // zero source instead: fp32 512^3 R2C y backward 228 -> 212 us, 256^3 neutral;
      // profiles/r5/ab/ymask)
      cx<T> v = czero<T>();
      if (base != kNoBase && b < zl) v = cvt<T>(ld_stick<Plain>(in + (base + z0 + b)));
      return v;
    } else {
      long long base;
      if (!ce.find(pos, base) || b >= zl) return czero<T>();
      return cvt<T>(ld_stream(&in[base + z0 + b]));
    }
  };
  // the x = 0 column of an R2C transform: gathered into LDS, hermitian fill
  auto stage_x0 = [&]() {
    zero_lds(lds, eng.input_elems());
    __syncthreads();
    gather_to_lds(lds, ce.ne * zl, [&](int idx) {
      const int e = idx / zl, zz = idx - e * zl;
      return cvt<T>(ld_stream(&in[ce.cBase[e] + z0 + zz]));
    }, [&](int idx) {
      const int e = idx / zl, zz = idx - e * zl;
      return eng.in_at(zz, ce.cY[e]);
    });
    __syncthreads();
    hermitian_lines(eng, lds, 0, B, n);
  };
  if constexpr (Eng::kBatchedCopy) {
    // run-time engines: stage either input path, then one FFT
    if (!x0) {
      eng.stage(lds, load);
      __syncthreads();
    } else {
      stage_x0();
    }
    eng.lds_to_lds(lds, tw);
  } else if (!x0) {
    eng.global_to_lds(lds, tw, load);
  } else {
    stage_x0();
    eng.lds_to_lds(lds, tw);
  }
  // rows of [z][column][y] are contiguous: coalesced copy-out
  copy_out<Eng>(lds, zl * n, [&](int idx) {
    const int b = idx / n;
    return eng.out_at(b, idx - b * n);
  }, [&](int idx, cx<T> v) {
    const int b = idx / n;
    st_inter(&inter[static_cast<long long>(z0 + b) * a.interZStride + inter_row(a, c) + idx - b * n], v);
  });
}

// Forward y stage, line-fast engine: lanes read rows of the intermediate and
// write each stick's z-run of this plane block directly (consecutive lanes ->
// consecutive z of one stick); no LDS staging on either side.
template <class Eng, typename T, typename BT>
__global__ void __launch_bounds__(Eng::kBlock)
    y_forward_kernel(Eng eng, YArgs a, const cx<T>* __restrict__ inter, BT* __restrict__ out,
                     const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, inter, out);
  const int B = eng.lines();
  const int n = eng.n();
  const int c = a.colBegin + y_tile_col();
  const int z0 = a.zBegin + y_tile_zblock() * B;
  const int zl = min(B, a.L - z0);
  constexpr bool kTable = y_table<Eng, has_store_pos<Eng>::value>();
  const ColEntries<Eng> ce(eng, a, lds, c, true, kTable);
  const RowSrc<cx<T>> rows{inter + static_cast<long long>(z0) * a.interZStride + inter_row(a, c),
                           a.interZStride};
  if constexpr (kTable) {
    // compile-time engines: the stick bases of the lane's output positions are
    // read from the y -> base table before the FFT (their LDS latency overlaps
    // the row loads); the stores then need no descriptor search per element
    using F = typename Eng::F;
    long long bases[F::kStoreSlots];
    F::for_each_store_pos([&](int i, int pos) { bases[i] = ce.yBase[pos]; });
    int slot = 0;
    stage_rows(eng, lds, zl, n, rows);
    eng.lds_to_global(lds, tw, [&](int b, int, cx<T> v) {
      const long long base = bases[slot++];
      if (base != kNoBase && b < zl) st_stream(&out[base + z0 + b], cvt<typename BT::value_type>(v));
    });
    return;
  }
  auto store = [&](int b, int pos, cx<T> v) {
    long long base;
    if (ce.find(pos, base) && b < zl) st_stream(&out[base + z0 + b], cvt<typename BT::value_type>(v));
  };
  stage_rows(eng, lds, zl, n, rows);
  eng.lds_to_global(lds, tw, store);
}

// x stage column lookup: every x of [0, nFreq) holds a column (e.g. a sphere
// of radius N/2) -> colX is the identity and no table is built; otherwise the
// workgroup stages the x -> column table in LDS. The table build is a
// dependent global load plus two barriers in front of every workgroup's main
// loads, so the dense case skips it.
__device__ __forceinline__ bool x_dense(const XArgs& a) { return a.ncols == a.nFreq; }
__device__ __forceinline__ void build_xcol(const XArgs& a, int* xCol, int count) {
  if (x_dense(a)) return;
  for (int x = threadIdx.x; x < count; x += blockDim.x) xCol[x] = -1;
  __syncthreads();
  for (int c = threadIdx.x; c < a.ncols; c += blockDim.x) xCol[a.colX[c]] = c;
  __syncthreads();
}
__device__ __forceinline__ int xcol_of(const XArgs& a, const int* xCol, int x) {
  return x_dense(a) ? (x < a.nFreq ? x : -1) : xCol[x];
}

// Packed-real C2R with the pre-pass folded into the first FFT pass's loads
// (compile-time engines): 66.9 -> 54.8 us at 256^3 fp64, R2C bench +2% fp64,
// +3% fp32 (profiles/r2_s1/shape_ab.txt); the run-time engines stage the
// pre-pass in LDS.

// ---------------------------------------------------------------- x stage
// Backward x stage with the line-fast engine: lane (line = row y, pos = x)
// reads column x of the intermediate (consecutive lanes -> consecutive y),
// zero for x without sticks; C2R completes the row by hermitian symmetry on
// the fly. The result is written row-contiguous from LDS.
template <class Eng, typename T, bool R2C>
__global__ void __launch_bounds__(Eng::kBlock)
    x_backward_kernel(Eng eng, XArgs a, const cx<T>* __restrict__ inter, void* __restrict__ space,
                      const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, inter, space);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, n);
  const cx<T>* src = inter + static_cast<long long>(zl) * a.interZStride + y0;
  const int yl = min(B, a.Y - y0);
  // kernel arguments the per-element loads use, pinned in scalar registers up
  // front (left to the compiler, their scalar loads were sunk into every
  // element's branch, each waited out before that element's load could issue)
  const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
  const int dense = pin_uniform(x_dense(a) ? 1 : 0);
  auto col_of = [&](int x) { return dense ? (x < nFreq ? x : -1) : xCol[x]; };
  auto load = [&](int b, int pos) -> cx<T> {
    if (b >= yl) return czero<T>();
    if (R2C && pos >= nFreq) {
      const int c = col_of(n - pos);
      return c < 0 ? czero<T>() : conj(ld_inter(&src[c * rowStride + b]));
    }
    const int c = col_of(pos);
    return c < 0 ? czero<T>() : ld_inter(&src[c * rowStride + b]);
  };
  const long long row0 = (static_cast<long long>(zl) * a.Y + y0) * n;
  eng.global_to_lds(lds, tw, load);
  copy_out<Eng>(lds, yl * n, [&](int idx) {
    const int b = idx / n;
    return eng.out_at(b, idx - b * n);
  }, [&](int idx, cx<T> v) {
    if (R2C)
      st_stream_real(&static_cast<T*>(space)[row0 + idx], v.x);
    else
      st_stream(&static_cast<cx<T>*>(space)[row0 + idx], v);
  });
}

// Forward x stage, line-fast engine: lanes read row segments of the space
// domain and write the columns that hold sticks straight into [z][column][y]
// (consecutive lanes -> consecutive y); R2C reads real rows.
template <class Eng, typename T, bool R2C>
__global__ void __launch_bounds__(Eng::kBlock)
    x_forward_kernel(Eng eng, XArgs a, const void* __restrict__ space, cx<T>* __restrict__ inter,
                     const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, space, inter);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, n);
  const int yl = min(B, a.Y - y0);
  cx<T>* dst = inter + static_cast<long long>(zl) * a.interZStride + y0;
  const long long row0 = (static_cast<long long>(zl) * a.Y + y0) * n;
  // arguments of the per-element stores pinned in scalar registers (see x_backward_kernel)
  const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
  const int dense = pin_uniform(x_dense(a) ? 1 : 0);
  auto store = [&](int b, int pos, cx<T> v) {
    const int c = dense ? (pos < nFreq ? pos : -1) : xCol[pos];
    if (c >= 0 && b < yl) st_inter(&dst[c * rowStride + b], v);
  };
  if constexpr (R2C)
    stage_rows(eng, lds, yl, n, RowSrc<T>{static_cast<const T*>(space) + row0, n});
  else
    stage_rows(eng, lds, yl, n, RowSrc<cx<T>>{static_cast<const cx<T>*>(space) + row0, n});
  eng.lds_to_global(lds, tw, store);
}

// Fused local-operator x stage (C2C): inverse x FFT of the tile's rows, multiply
// by the real potential V[z][y][x], forward x FFT, all in LDS; the space domain
// is neither written nor read. forward_twin(eng) is the forward engine that
// runs on the LDS lines of the backward engine `eng`: same lines, line stride,
// padding and threads. The host makes it and passes it as a kernel argument of
// its own (a run-time plan copied inside the kernel would live in scratch: its
// radix table is indexed).
template <typename T, int N, bool LF, bool TwPre>
__host__ __device__ inline CtEngS<T, N, -1, LF, TwPre, +1> forward_twin(const CtEng<T, N, +1, LF, TwPre>&) {
  using FB = typename CtEng<T, N, +1, LF, TwPre>::F;
  using FF = typename CtEngS<T, N, -1, LF, TwPre, +1>::F;
  static_assert(FB::B == FF::B && FB::LS == FF::LS && FB::PS == FF::PS && FB::NT == FF::NT,
                "x apply: the inverse and forward engines must share one LDS layout");
  return {};
}
template <typename T, bool LF>
__host__ __device__ inline RtEng<T, -1, LF> forward_twin(const RtEng<T, +1, LF>& e) {
  return RtEng<T, -1, LF>{e.p};
}
template <typename T>
__host__ __device__ inline BlueEng<T, -1> forward_twin(const BlueEng<T, +1>& e) {
  return BlueEng<T, -1>{e.pm, e.nn, e.chirp, e.filt, e.twm};
}

// lds[dst(idx)] = lds[src(idx)] * v[idx] for idx in [0, total): lanes walk the
// rows contiguously (the order of copy_out), so the loads of V coalesce and a
// wave's LDS accesses are consecutive elements of one line. With the access
// rules of tools/lds_bank_model.py the writes are conflict-free in both
// precisions and the fp32 reads too; the fp64 reads of padded lines take 8
// cycles per wave instead of 4 (a pad element falls inside every ds_read_b128
// lane group), as in copy_out: 8 reads per lane, about 2 of the stage's 123 us
// at 256^3 (profiles/r7/apply_local). kApplyUnroll loads of V are in flight per
// lane. No LDS race: lane idx reads src(idx) and writes dst(idx), and the kernel
// calls this with src = the inverse engine's out_at and dst = the forward
// engine's in_at, which are either the same slot (compile-time engines: out_at
// == in_at on one layout, which the static_assert of forward_twin guarantees;
// in-place run-time plans; Bluestein) or slots of two disjoint LDS regions
// (ping-pong run-time plans with an odd pass count). A shared shape whose out_at
// and in_at differ inside one region would need a barrier-separated copy instead.
// Stream: V is read once (non-temporal); plain loads for a potential shared by a
// batch.
constexpr int kApplyUnroll = 8;
template <bool Stream, typename T, class Src, class Dst>
__device__ __forceinline__ void scale_rows(cx<T>* lds, const T* __restrict__ v, int total, Src src, Dst dst) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kApplyUnroll) {
    T w[kApplyUnroll];
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        if constexpr (Stream) w[u] = ld_stream_real(v + idx);
        else w[u] = v[idx];
      }
    }
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) lds[dst(idx)] = scale(lds[src(idx)], w[u]);
    }
  }
}

// In place on the [z][column][y] intermediate: a workgroup owns the tile of
// x_backward_kernel / x_forward_kernel (plane z, rows y0..y0+B, every column).
// Invariant that makes the in-place update safe: the inverse FFT's first pass
// reads every element of the tile before the forward FFT stores any, with the
// multiply's barriers in between, and no other workgroup touches the tile.
template <class Eng, class Fwd, typename T, bool StreamV>
__global__ void __launch_bounds__(Eng::kBlock)
    x_apply_kernel(Eng eng, Fwd fwd, XArgs a, const T* __restrict__ potential, cx<T>* inter,
                   const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, potential, inter);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, n);
  cx<T>* tile = inter + static_cast<long long>(zl) * a.interZStride + y0;
  const int yl = min(B, a.Y - y0);
  // per-element arguments pinned in scalar registers (see x_backward_kernel)
  const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
  const int dense = pin_uniform(x_dense(a) ? 1 : 0);
  auto col_of = [&](int x) { return dense ? (x < nFreq ? x : -1) : xCol[x]; };
  auto load = [&](int b, int pos) -> cx<T> {
    if (b >= yl) return czero<T>();
    const int c = col_of(pos);
    return c < 0 ? czero<T>() : ld_inter(&tile[c * rowStride + b]);
  };
  auto store = [&](int b, int pos, cx<T> v) {
    const int c = col_of(pos);
    if (c >= 0 && b < yl) st_inter(&tile[c * rowStride + b], v);
  };
  eng.global_to_lds(lds, tw, load);  // rows at out_at(b, x); ends with a barrier
  const T* v = potential + (static_cast<long long>(zl) * a.Y + y0) * n;
  scale_rows<StreamV>(lds, v, yl * n, [&](int idx) {
    const int b = idx / n;
    return eng.out_at(b, idx - b * n);
  }, [&](int idx) {
    const int b = idx / n;
    return fwd.in_at(b, idx - b * n);
  });
  __syncthreads();
  fwd.lds_to_global(lds, tw, store);
}

// In-place multiply of the space domain by a real potential (the unfused
// local-operator path: R2C transforms and long x lines): E = cx<T> or T.
template <typename E, typename T>
__global__ void __launch_bounds__(256)
    space_scale_kernel(E* __restrict__ space, const T* __restrict__ potential, long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    const T w = ld_stream_real(potential + i);
    if constexpr (std::is_same<E, T>::value)
      st_stream_real(space + i, ld_stream_real(space + i) * w);
    else
      st_stream(space + i, scale(ld_stream(space + i), w));
  }
}

// Fused reciprocal-space operator z stage (simple sticks): forward z FFT of the
// block's sticks into LDS, values = scale * coefficient and coefficient *= K on
// the sparse set (zero elsewhere), (0,0)-stick hermitian fill, inverse z FFT,
// store to the same stick addresses; the sparse values make no round trip
// through memory. `fwd` is forward_twin(eng): the forward engine on the LDS
// lines of the backward stage's engine `eng`.
//
// The multiply walks the B x n LDS elements with z fastest, so a wave's lanes
// follow the z-runs of a stick: consecutive value indices, coalesced loads of K
// and stores of `values`. kApplyUnroll loads of K are in flight per lane. No LDS
// race: lane idx reads fwd.out_at and writes eng.in_at of its own element,
// which are the same slot (compile-time engines on one layout, in-place run-time
// plans, Bluestein) or slots of two disjoint regions (ping-pong run-time plans
// with an odd pass count), as in scale_rows.
//
// In place on the stick side. Invariant that makes it safe: the forward FFT has
// loaded every element of the block's sticks before the inverse FFT stores any
// (barriers in between), and no other workgroup touches these sticks.
template <typename T, bool Cplx>
__device__ __forceinline__ cx<T> ld_kernel(const T* __restrict__ k, long long i) {
  if constexpr (Cplx) return ld_stream(reinterpret_cast<const cx<T>*>(k) + i);
  else return mk<T>(ld_stream_real(k + i), T(0));
}

template <class Eng, class Fwd, typename T, bool Cplx, bool Plain>
__global__ void __launch_bounds__(Eng::kBlock)
    z_reciprocal_kernel(Eng eng, Fwd fwd, ZArgs a, cx<T>* sticks, const T* __restrict__ kern,
                        cx<T>* __restrict__ values, T scale, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int n = eng.n();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const int nl = min(B, a.numSticks - s0);
  const ZSeg seg(a.single, a.stickStride, a.zTab,
                 reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), n);
  StickDesc* d = reinterpret_cast<StickDesc*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  for (int b = threadIdx.x; b < nl; b += blockDim.x) d[b] = a.desc[s0 + b];
  // result at fwd.out_at(b, z); ends with a barrier (which also publishes d)
  fwd.global_to_lds(lds, tw, [&](int b, int pos) -> cx<T> {
    if (b >= nl) return czero<T>();
    return ld_stream(&sticks[seg.at(s0 + b, pos)]);
  });
  const bool keep = pin_uniform(values != nullptr ? 1 : 0) != 0;
  const int total = B * n;
  for (int base = threadIdx.x; base < total; base += blockDim.x * kApplyUnroll) {
    cx<T> w[kApplyUnroll];
    int vi[kApplyUnroll];
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      vi[u] = -1;
      if (idx < total) {
        const int b = idx / n, z = idx - b * n;
        if (b < nl) {
          const StickDesc& q = d[b];
          const int j = desc_offset(q, z);
          if (j >= 0) {
            vi[u] = q.valueStart + j;
            w[u] = ld_kernel<T, Cplx>(kern, vi[u]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const int b = idx / n, z = idx - b * n;
        cx<T> r = czero<T>();
        if (vi[u] >= 0) {
          const cx<T> v = spfft::scale(lds[fwd.out_at(b, z)], scale);
          if (keep) st_values(&values[vi[u]], v);
          if constexpr (Cplx) r = cmul(v, w[u]);
          else r = spfft::scale(v, w[u].x);
        }
        lds[eng.in_at(b, z)] = r;
      }
    }
  }
  __syncthreads();
  if (a.zeroStick >= s0 && a.zeroStick < s0 + nl) hermitian_lines_inline(eng, lds, a.zeroStick - s0, 1, n);
  eng.lds_to_global(lds, tw, [&](int b, int pos, cx<T> v) {
    if (b < nl) st_stick<Plain>(&sticks[seg.at(s0 + b, pos)], v);
  });
}

// Batched launch of the kernel above (the pairs of
// multi_transform_accumulate_fock): blockIdx.z selects the member, whose stick
// array (in place) is ZArgs::batch.out and whose kernel K is ZArgs::batch.in;
// the index tables are shared, and there is no values output. A kernel of its
// own, not a shared inlined body: with the body in a function the single
// launch's kernels took 12 to 42 more VGPRs (N = 128 fp64: 86 -> 128).
template <class Eng, class Fwd, typename T, bool Cplx, bool Plain>
__global__ void __launch_bounds__(Eng::kBlock)
    z_reciprocal_batch_kernel(Eng eng, Fwd fwd, ZArgs a, T scale, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  cx<T>* sticks = static_cast<cx<T>*>(a.batch.out[blockIdx.z]);
  const T* __restrict__ kern = static_cast<const T*>(a.batch.in[blockIdx.z]);
  const int B = eng.lines();
  const int n = eng.n();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const int nl = min(B, a.numSticks - s0);
  const ZSeg seg(a.single, a.stickStride, a.zTab,
                 reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), n);
  StickDesc* d = reinterpret_cast<StickDesc*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  for (int b = threadIdx.x; b < nl; b += blockDim.x) d[b] = a.desc[s0 + b];
  // result at fwd.out_at(b, z); ends with a barrier (which also publishes d)
  fwd.global_to_lds(lds, tw, [&](int b, int pos) -> cx<T> {
    if (b >= nl) return czero<T>();
    return ld_stream(&sticks[seg.at(s0 + b, pos)]);
  });
  const int total = B * n;
  for (int base = threadIdx.x; base < total; base += blockDim.x * kApplyUnroll) {
    cx<T> w[kApplyUnroll];
    int vi[kApplyUnroll];
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      vi[u] = -1;
      if (idx < total) {
        const int b = idx / n, z = idx - b * n;
        if (b < nl) {
          const StickDesc& q = d[b];
          const int j = desc_offset(q, z);
          if (j >= 0) {
            vi[u] = q.valueStart + j;
            w[u] = ld_kernel<T, Cplx>(kern, vi[u]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const int b = idx / n, z = idx - b * n;
        cx<T> r = czero<T>();
        if (vi[u] >= 0) {
          const cx<T> v = spfft::scale(lds[fwd.out_at(b, z)], scale);
          if constexpr (Cplx) r = cmul(v, w[u]);
          else r = spfft::scale(v, w[u].x);
        }
        lds[eng.in_at(b, z)] = r;
      }
    }
  }
  __syncthreads();
  if (a.zeroStick >= s0 && a.zeroStick < s0 + nl) hermitian_lines_inline(eng, lds, a.zeroStick - s0, 1, n);
  eng.lds_to_global(lds, tw, [&](int b, int pos, cx<T> v) {
    if (b < nl) st_stick<Plain>(&sticks[seg.at(s0 + b, pos)], v);
  });
}

// Reciprocal fan-out z stage (multi_transform_reciprocal_fan_out, simple
// sticks): one forward z FFT of member 0's sticks feeds an inverse z FFT per
// member. c = scale * coefficient is parked on the sparse set (zero elsewhere)
// in a second LDS region `hold` behind the launch's other LDS (byte offset
// holdOffset), element (b, z) at hold[b * n + z]; `values` receives c when
// given. Per member m the line region gets K_m * c, the (0,0) stick is filled
// and the inverse FFT stores to the member's stick array (ZArgs::batch.out[m],
// kernel ZArgs::batch.in[m]). One workgroup owns a block of sticks and loops
// over the members; the grid is that of z_reciprocal_kernel.
//
// Member 0 is written in place over the input, so it runs last; the only loads
// of stick array 0 are those of the forward FFT, barriers before any store.
// LDS: lane idx of the walk owns hold[idx] and the line slot of its element in
// every loop (as in z_reciprocal_kernel), and barriers separate the walks from
// the FFTs. Consecutive lanes touch consecutive 16- or 8-byte elements of
// `hold`: conflict free.
template <class Eng, class Fwd, typename T, bool Cplx, bool Plain>
__global__ void __launch_bounds__(Eng::kBlock)
    z_reciprocal_fan_out_kernel(Eng eng, Fwd fwd, ZArgs a, cx<T>* __restrict__ values, T scale, int holdOffset,
                                const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  cx<T>* hold = reinterpret_cast<cx<T>*>(spfftSmem + holdOffset);
  const int members = pin_uniform(a.batch.count);
  const int B = eng.lines();
  const int n = eng.n();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const int nl = min(B, a.numSticks - s0);
  const ZSeg seg(a.single, a.stickStride, a.zTab,
                 reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), n);
  StickDesc* d = reinterpret_cast<StickDesc*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  for (int b = threadIdx.x; b < nl; b += blockDim.x) d[b] = a.desc[s0 + b];
  {
    const cx<T>* __restrict__ src = static_cast<const cx<T>*>(a.batch.out[0]);
    // result at fwd.out_at(b, z); ends with a barrier (which also publishes d)
    fwd.global_to_lds(lds, tw, [&](int b, int pos) -> cx<T> {
      if (b >= nl) return czero<T>();
      return ld_stream(&src[seg.at(s0 + b, pos)]);
    });
  }
  const bool keep = pin_uniform(values != nullptr ? 1 : 0) != 0;
  const int total = B * n;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int b = idx / n, z = idx - b * n;
    cx<T> c = czero<T>();
    if (b < nl) {
      const StickDesc& q = d[b];
      const int j = desc_offset(q, z);
      if (j >= 0) {
        c = spfft::scale(lds[fwd.out_at(b, z)], scale);
        if (keep) st_values(&values[q.valueStart + j], c);
      }
    }
    hold[idx] = c;
  }
  __syncthreads();
  for (int step = 1; step <= members; ++step) {
    const int m = step == members ? 0 : step;
    cx<T>* sticks = static_cast<cx<T>*>(a.batch.out[m]);
    const T* __restrict__ kern = static_cast<const T*>(a.batch.in[m]);
    // opaque per member: twiddle loads and the lanes' stick offsets, hoisted out
    // of the member loop, stay live across it and cost registers
    const cx<T>* twm = tw;
    int s0m = s0;
    asm volatile("" : "+s"(twm), "+s"(s0m));
    for (int base = threadIdx.x; base < total; base += blockDim.x * kApplyUnroll) {
      cx<T> w[kApplyUnroll];
      int vi[kApplyUnroll];
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) {
        const int idx = base + u * static_cast<int>(blockDim.x);
        vi[u] = -1;
        if (idx < total) {
          const int b = idx / n, z = idx - b * n;
          if (b < nl) {
            const StickDesc& q = d[b];
            const int j = desc_offset(q, z);
            if (j >= 0) {
              vi[u] = q.valueStart + j;
              w[u] = ld_kernel<T, Cplx>(kern, vi[u]);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) {
        const int idx = base + u * static_cast<int>(blockDim.x);
        if (idx < total) {
          const int b = idx / n, z = idx - b * n;
          cx<T> r = czero<T>();
          if (vi[u] >= 0) {
            const cx<T> v = hold[idx];
            if constexpr (Cplx) r = cmul(v, w[u]);
            else r = spfft::scale(v, w[u].x);
          }
          lds[eng.in_at(b, z)] = r;
        }
      }
    }
    __syncthreads();
    if (a.zeroStick >= s0 && a.zeroStick < s0 + nl) hermitian_lines_inline(eng, lds, a.zeroStick - s0, 1, n);
    eng.lds_to_global(lds, twm, [&](int b, int pos, cx<T> v) {
      if (b < nl) st_stick<Plain>(&sticks[seg.at(s0m + b, pos)], v);
    });
    __syncthreads();  // the inverse FFT has read its lines before the next member's fill
  }
}

// Reciprocal fan-in z stage (multi_transform_reciprocal_fan_in): per member m in
// list order the forward z FFT of the block's sticks of ZArgs::batch.out[m],
// then acc += K_m * (scale * coefficient) on the sparse set (K_m =
// ZArgs::batch.in[m]); the sum's (0,0) stick is filled and one inverse z FFT
// stores to batch.out[0]. `acc` is the second LDS region of the fan-out kernel
// (same layout, same lane ownership: no atomics, no race, and a sum order fixed
// by the member order alone). The stick arrays of the members m > 0 are only
// read; member 0's is written after the last load of it (barriers in between).
template <class Eng, class Fwd, typename T, bool Cplx, bool Plain>
__global__ void __launch_bounds__(Eng::kBlock)
    z_reciprocal_fan_in_kernel(Eng eng, Fwd fwd, ZArgs a, T scale, int holdOffset, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  cx<T>* acc = reinterpret_cast<cx<T>*>(spfftSmem + holdOffset);
  const int members = pin_uniform(a.batch.count);
  const int B = eng.lines();
  const int n = eng.n();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const int nl = min(B, a.numSticks - s0);
  const ZSeg seg(a.single, a.stickStride, a.zTab,
                 reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), n);
  StickDesc* d = reinterpret_cast<StickDesc*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  for (int b = threadIdx.x; b < nl; b += blockDim.x) d[b] = a.desc[s0 + b];
  const int total = B * n;
  for (int m = 0; m < members; ++m) {
    const cx<T>* __restrict__ src = static_cast<const cx<T>*>(a.batch.out[m]);
    const T* __restrict__ kern = static_cast<const T*>(a.batch.in[m]);
    // the previous member's walk has read its coefficients before these lines are reused
    if (m > 0) __syncthreads();
    // opaque per member: twiddle loads and the lanes' stick offsets, hoisted out
    // of the member loop, stay live across it and cost registers
    const cx<T>* twm = tw;
    int s0m = s0;
    asm volatile("" : "+s"(twm), "+s"(s0m));
    // result at fwd.out_at(b, z); ends with a barrier (which also publishes d)
    fwd.global_to_lds(lds, twm, [&](int b, int pos) -> cx<T> {
      if (b >= nl) return czero<T>();
      return ld_stream(&src[seg.at(s0m + b, pos)]);
    });
    for (int base = threadIdx.x; base < total; base += blockDim.x * kApplyUnroll) {
      cx<T> w[kApplyUnroll];
      int vi[kApplyUnroll];
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) {
        const int idx = base + u * static_cast<int>(blockDim.x);
        vi[u] = -1;
        if (idx < total) {
          const int b = idx / n, z = idx - b * n;
          if (b < nl) {
            const StickDesc& q = d[b];
            const int j = desc_offset(q, z);
            if (j >= 0) {
              vi[u] = q.valueStart + j;
              w[u] = ld_kernel<T, Cplx>(kern, vi[u]);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) {
        const int idx = base + u * static_cast<int>(blockDim.x);
        if (idx < total) {
          const int b = idx / n, z = idx - b * n;
          cx<T> r = czero<T>();
          if (vi[u] >= 0) {
            const cx<T> v = spfft::scale(lds[fwd.out_at(b, z)], scale);
            if constexpr (Cplx) r = cmul(v, w[u]);
            else r = spfft::scale(v, w[u].x);
          }
          if (m > 0) {
            const cx<T> s = acc[idx];
            r = mk<T>(s.x + r.x, s.y + r.y);
          }
          acc[idx] = r;
        }
      }
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int b = idx / n, z = idx - b * n;
    lds[eng.in_at(b, z)] = acc[idx];
  }
  __syncthreads();
  if (a.zeroStick >= s0 && a.zeroStick < s0 + nl) hermitian_lines_inline(eng, lds, a.zeroStick - s0, 1, n);
  cx<T>* sticks = static_cast<cx<T>*>(a.batch.out[0]);
  eng.lds_to_global(lds, tw, [&](int b, int pos, cx<T> v) {
    if (b < nl) st_stick<Plain>(&sticks[seg.at(s0 + b, pos)], v);
  });
}

// Value fan-out z stage (multi_transform_accumulate_density_fan / apply_local_fan,
// simple sticks, C2C): one set of frequency values feeds an inverse z FFT per
// member. A workgroup owns a block of sticks of one member m = blockIdx.z (the
// grid of the batched backward z stage): its line region gets K_m * value on
// the sparse set and zero elsewhere (K_m = ZArgs::batch.in[m]; null is the
// identity, a branch that is uniform over the workgroup), and the inverse FFT
// stores to the member's stick array ZArgs::batch.out[m]. The members'
// workgroups read the same values (a few KB per block, from L2 or the Infinity
// Cache after the first), so nothing is parked in a second LDS region and the
// kernel keeps the LDS footprint of the backward z stage. A loop over the
// members inside one workgroup was measured first and lost to the composition
// on small grids, where few workgroups each ran the members' FFTs one after
// another (profiles/r13/values_fan). `values` is only read and no stick array
// is read. There is no hermitian fill: the dispatch takes this path for C2C
// plans only. Compile-time engines load K_m * value into the registers of the
// first FFT pass (the fast path of z_backward_desc_kernel); run-time and
// Bluestein engines fill the line region in LDS first.
constexpr int kFanOutUnroll = 4;  // value and kernel loads in flight per lane
template <class Eng, typename T, bool Cplx, bool Plain>
__global__ void __launch_bounds__(Eng::kBlock)
    z_values_fan_out_kernel(Eng eng, ZArgs a, const cx<T>* __restrict__ values, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  const int m = blockIdx.z;  // < a.batch.count (the launcher's grid)
  cx<T>* __restrict__ sticks = static_cast<cx<T>*>(a.batch.out[m]);
  const T* __restrict__ kern = static_cast<const T*>(a.batch.in[m]);
  const bool ident = kern == nullptr;
  const int B = eng.lines();
  const int n = eng.n();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const int nl = min(B, a.numSticks - s0);
  const ZSeg seg(a.single, a.stickStride, a.zTab,
                 reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), n);
  auto store = [&](int b, int pos, cx<T> x) {
    if (b < nl) st_stick<Plain>(&sticks[seg.at(s0 + b, pos)], x);
  };
  StickDesc* d = reinterpret_cast<StickDesc*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  for (int b = threadIdx.x; b < nl; b += blockDim.x) d[b] = a.desc[s0 + b];
  __syncthreads();
  if constexpr (!Eng::kBatchedCopy) {
    // the lane's own stick descriptor in registers, as in z_backward_desc_kernel
    const int lb = Eng::F::lane_line();
    StickDesc q = d[lb < nl ? lb : 0];
    int z0 = q.z0, len0 = q.len0, z1 = q.z1, len1 = q.count - q.len0, vs = q.valueStart;
    if (lb >= nl) len0 = len1 = 0;
    asm volatile("" : "+v"(z0), "+v"(len0), "+v"(z1), "+v"(len1), "+v"(vs));
    const cx<T>* vals = values + vs;
    eng.global_to_global(lds, tw, [&](int, int z) -> cx<T> {
      const unsigned j0 = static_cast<unsigned>(z - z0), j1 = static_cast<unsigned>(z - z1);
      const bool in0 = j0 < static_cast<unsigned>(len0);
      const bool in1 = j1 < static_cast<unsigned>(len1);
      if (!(in0 || in1)) return czero<T>();
      const int j = in0 ? static_cast<int>(j0) : len0 + static_cast<int>(j1);
      // (default cache policy: the other members' workgroups read the same values)
      const cx<T> v = ld_values(&vals[j]);
      if (ident) return v;
      const cx<T> w = ld_kernel<T, Cplx>(kern, vs + j);
      if constexpr (Cplx) return cmul(v, w);
      else return spfft::scale(v, w.x);
    }, store);
  } else {
    const int total = B * n;
    for (int base = threadIdx.x; base < total; base += blockDim.x * kFanOutUnroll) {
      cx<T> w[kFanOutUnroll], v[kFanOutUnroll];
      int vi[kFanOutUnroll];
#pragma unroll
      for (int u = 0; u < kFanOutUnroll; ++u) {
        const int idx = base + u * static_cast<int>(blockDim.x);
        vi[u] = -1;
        if (idx < total) {
          const int b = idx / n, z = idx - b * n;
          if (b < nl) {
            const StickDesc& q = d[b];
            const int j = desc_offset(q, z);
            if (j >= 0) {
              vi[u] = q.valueStart + j;
              v[u] = ld_values(&values[vi[u]]);
              if (!ident) w[u] = ld_kernel<T, Cplx>(kern, vi[u]);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kFanOutUnroll; ++u) {
        const int idx = base + u * static_cast<int>(blockDim.x);
        if (idx < total) {
          const int b = idx / n, z = idx - b * n;
          cx<T> r = czero<T>();
          if (vi[u] >= 0) {
            if (ident) r = v[u];
            else if constexpr (Cplx) r = cmul(v[u], w[u]);
            else r = spfft::scale(v[u], w[u].x);
          }
          lds[eng.in_at(b, z)] = r;
        }
      }
    }
    __syncthreads();
    eng.lds_to_global(lds, tw, store);
  }
}

// Value fan-in z stage (multi_transform_apply_local_fan): per member m in list
// order the forward z FFT of the block's sticks of ZArgs::batch.out[m], then
// acc += L_m * (scale * coefficient) on the sparse set (L_m = ZArgs::batch.in[m];
// null is the identity); after the loop one coalesced store of acc to `output`
// through the stick descriptors. There is no inverse FFT. `acc` is a second LDS
// region behind the launch's other LDS (byte offset accOffset), element (b, z)
// at acc[b * n + z], with the lane ownership of z_reciprocal_fan_in_kernel: lane
// idx of the walk owns acc[idx] in every member's walk and in the store, so
// there are no atomics and no race, and the sum order is the member order. The
// stick arrays are only read.
template <class Eng, class Fwd, typename T, bool Cplx>
__global__ void __launch_bounds__(Eng::kBlock)
    z_values_fan_in_kernel(Eng eng, Fwd fwd, ZArgs a, cx<T>* __restrict__ output, T scale, int accOffset,
                           const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  cx<T>* acc = reinterpret_cast<cx<T>*>(spfftSmem + accOffset);
  const int members = pin_uniform(a.batch.count);
  const int B = eng.lines();
  const int n = eng.n();
  const int s0 = a.stickBegin + block_tile_x() * B;
  const int nl = min(B, a.numSticks - s0);
  const ZSeg seg(a.single, a.stickStride, a.zTab,
                 reinterpret_cast<char*>(lds) + zseg_lds_offset(eng.lds_bytes(), B), n);
  StickDesc* d = reinterpret_cast<StickDesc*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  for (int b = threadIdx.x; b < nl; b += blockDim.x) d[b] = a.desc[s0 + b];
  const int total = B * n;
  for (int m = 0; m < members; ++m) {
    const cx<T>* __restrict__ src = static_cast<const cx<T>*>(a.batch.out[m]);
    const T* __restrict__ kern = static_cast<const T*>(a.batch.in[m]);
    const bool ident = kern == nullptr;
    // the previous member's walk has read its coefficients before these lines are reused
    if (m > 0) __syncthreads();
    // opaque per member, as in the fan-out kernel
    const cx<T>* twm = tw;
    int s0m = s0;
    asm volatile("" : "+s"(twm), "+s"(s0m));
    // result at fwd.out_at(b, z); ends with a barrier (which also publishes d)
    fwd.global_to_lds(lds, twm, [&](int b, int pos) -> cx<T> {
      if (b >= nl) return czero<T>();
      return ld_stream(&src[seg.at(s0m + b, pos)]);
    });
    for (int base = threadIdx.x; base < total; base += blockDim.x * kApplyUnroll) {
      cx<T> w[kApplyUnroll];
      int vi[kApplyUnroll];
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) {
        const int idx = base + u * static_cast<int>(blockDim.x);
        vi[u] = -1;
        if (idx < total) {
          const int b = idx / n, z = idx - b * n;
          if (b < nl) {
            const StickDesc& q = d[b];
            const int j = desc_offset(q, z);
            if (j >= 0) {
              vi[u] = q.valueStart + j;
              if (!ident) w[u] = ld_kernel<T, Cplx>(kern, vi[u]);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) {
        const int idx = base + u * static_cast<int>(blockDim.x);
        if (idx < total) {
          const int b = idx / n, z = idx - b * n;
          cx<T> r = czero<T>();
          if (vi[u] >= 0) {
            const cx<T> c = spfft::scale(lds[fwd.out_at(b, z)], scale);
            if (ident) r = c;
            else if constexpr (Cplx) r = cmul(c, w[u]);
            else r = spfft::scale(c, w[u].x);
          }
          if (m > 0) {
            const cx<T> s = acc[idx];
            r = mk<T>(s.x + r.x, s.y + r.y);
          }
          acc[idx] = r;
        }
      }
    }
  }
  // every lane stores the elements of acc it owns: no barrier in between
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int b = idx / n, z = idx - b * n;
    if (b < nl) {
      const StickDesc& q = d[b];
      const int j = desc_offset(q, z);
      if (j >= 0) st_values(&output[q.valueStart + j], acc[idx]);
    }
  }
}

// acc[i] += in[i] over `count` sparse values (composed value fan, identity L).
template <typename T>
__global__ void __launch_bounds__(256) values_add_kernel(cx<T>* acc, const cx<T>* __restrict__ in, long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
    acc[i] = mk<T>(acc[i].x + in[i].x, acc[i].y + in[i].y);
}

// acc[i] += in[i] * K[i] over `count` sparse values (the composed fan-in path).
template <typename T, bool Cplx>
__global__ void __launch_bounds__(256)
    values_scale_add_kernel(cx<T>* acc, const cx<T>* __restrict__ in, const T* __restrict__ kern, long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    const cx<T> w = ld_kernel<T, Cplx>(kern, i);
    cx<T> r;
    if constexpr (Cplx) r = cmul(in[i], w);
    else r = spfft::scale(in[i], w.x);
    acc[i] = mk<T>(acc[i].x + r.x, acc[i].y + r.y);
  }
}

// out[i] = in[i] * K[i] over `count` sparse values (the composed reciprocal-space
// operator path; out may be in); K real or complex.
template <typename T, bool Cplx>
__global__ void __launch_bounds__(256)
    values_scale_kernel(cx<T>* out, const cx<T>* in, const T* __restrict__ kern, long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    const cx<T> w = ld_kernel<T, Cplx>(kern, i);
    if constexpr (Cplx) out[i] = cmul(in[i], w);
    else out[i] = spfft::scale(in[i], w.x);
  }
}

// Fused density x stage (C2C): rho[z][y][x] += w |backward(values)[z][y][x]|^2
// with the inverse x FFT of the tile's rows in LDS; the space domain is neither
// written nor read. Weights of a batched launch, by value.
template <typename T>
struct DensityWeights {
  T w[kMaxBatch];
};
template <typename T>
__device__ __forceinline__ T norm2(cx<T> v) {
  return fma(v.x, v.x, v.y * v.y);
}

// rho[idx] = fma(w, |lds[src(idx)]|^2, rho[idx]) for idx in [0, total): lanes
// walk the rows contiguously (the order of copy_out), so the accesses of rho
// coalesce; kDensityUnroll loads of rho are in flight per lane before the first
// dependent store (the compiler may not move a load of rho over a store to it).
// The unroll is kept small: copy_out's fully unrolled tile on top of the rho
// values doubled the kernel's VGPRs against x_backward_kernel (N = 128 fp64:
// 140 against 69) and spilled at N = 1024. Stream: rho is read and written once
// per launch (non-temporal); plain accesses when the bands of a batch revisit
// the tile.
constexpr int kDensityUnroll = 4;
template <bool Stream, typename T, class Src>
__device__ __forceinline__ void density_rows(const cx<T>* lds, T* __restrict__ rho, T w, int total, Src src) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kDensityUnroll) {
    T r[kDensityUnroll];
#pragma unroll
    for (int u = 0; u < kDensityUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        if constexpr (Stream) r[u] = ld_stream_real(rho + idx);
        else r[u] = rho[idx];
      }
    }
#pragma unroll
    for (int u = 0; u < kDensityUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const T v = fma(w, norm2(lds[src(idx)]), r[u]);
        if constexpr (Stream) st_stream_real(rho + idx, v);
        else rho[idx] = v;
      }
    }
  }
}

// A workgroup owns the tile of x_backward_kernel (plane z, rows y0..y0+B, every
// column) and with it the rows of rho: no other workgroup of the launch touches
// them, so the update needs no atomics. The bands of a batched launch share
// rho, so they are not spread over blockIdx.z: the workgroup loops over them
// for its tile (intermediates from XArgs::batch.in), and lane idx updates the
// same elements of rho for every band, in band order (in registers for full
// tiles of compile-time engines, else in rho itself, where a band's update is
// ordered behind the previous one's by the lane's own program order): the
// sum order is fixed. StreamRho: the cache policy of the rho accesses (a template
// parameter: a run-time flag costs registers, profiles/r6/ntmerge). Batched:
// the band loop; a single-band launch runs the body once without it, with the
// register budget of x_backward_kernel.
template <class Eng, typename T, bool StreamRho, bool Batched>
__global__ void __launch_bounds__(Eng::kBlock)
    x_density_kernel(Eng eng, XArgs a, const cx<T>* __restrict__ inter, T* __restrict__ density,
                     DensityWeights<T> weights, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, n);
  const int yl = min(B, a.Y - y0);
  T* rho = density + (static_cast<long long>(zl) * a.Y + y0) * n;
  // inverse x FFT of band `interM`'s tile: rows at out_at(b, x); ends with a barrier
  auto fft = [&](const cx<T>* interM, const cx<T>* twM) {
    // per-element arguments pinned in scalar registers (see x_backward_kernel)
    const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
    const int dense = pin_uniform(x_dense(a) ? 1 : 0);
    auto col_of = [&](int x) { return dense ? (x < nFreq ? x : -1) : xCol[x]; };
    const cx<T>* src = interM + static_cast<long long>(zl) * a.interZStride + y0;
    auto load = [&](int b, int pos) -> cx<T> {
      if (b >= yl) return czero<T>();
      const int c = col_of(pos);
      return c < 0 ? czero<T>() : ld_inter(&src[c * rowStride + b]);
    };
    eng.global_to_lds(lds, twM, load);
  };
  auto row_at = [&](int idx) {
    const int b = idx / n;
    return eng.out_at(b, idx - b * n);
  };
  if constexpr (!Batched) {
    fft(inter, tw);
    density_rows<StreamRho>(lds, rho, weights.w[0], yl * n, row_at);
  } else {
    // the per-element arguments (in fft) and the twiddle table are pinned anew
    // for every band: as loop invariants, the FFT's column offsets and twiddles
    // were hoisted out of the band loop and stayed live across it (N = 256
    // fp64: 122 VGPRs with them hoisted, x_backward_kernel 66)
    auto band_fft = [&](int m) {
      const cx<T>* twM = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(tw)));
      if (m > 0) __syncthreads();  // the previous band's rows have been read
      fft(static_cast<const cx<T>*>(a.batch.in[m]), twM);
    };
    // A full tile of a compile-time engine has a compile-time number of elements
    // per lane: the bands' contributions are summed in registers and rho is
    // read and written once, instead of once per band through L2. 256^3 fp64, 8
    // bands: the call 1692 -> 1600 us (profiles/r8/density).
    if constexpr (!Eng::kBatchedCopy) {
      using F = typename Eng::F;
      constexpr bool kEven = (F::B * Eng::kN) % F::NT == 0;
      if (kEven && yl == F::B) {
        constexpr int kIters = kEven ? F::B * Eng::kN / F::NT : 1;
        T acc[kIters];
#pragma unroll
        for (int i = 0; i < kIters; ++i) acc[i] = T(0);
        for (int m = 0; m < a.batch.count; ++m) {
          band_fft(m);
          const T w = weights.w[m];
#pragma unroll
          for (int i = 0; i < kIters; ++i)
            acc[i] = fma(w, norm2(lds[row_at(static_cast<int>(threadIdx.x) + i * F::NT)]), acc[i]);
        }
#pragma unroll
        for (int i = 0; i < kIters; ++i) acc[i] += rho[static_cast<int>(threadIdx.x) + i * F::NT];
#pragma unroll
        for (int i = 0; i < kIters; ++i) rho[static_cast<int>(threadIdx.x) + i * F::NT] = acc[i];
        return;
      }
    }
    for (int m = 0; m < a.batch.count; ++m) {
      band_fft(m);
      density_rows<StreamRho>(lds, rho, weights.w[m], yl * n, row_at);
    }
  }
}

// Engines whose batched x density launch keeps the band loop inside the
// workgroup. The fp32 N = 1024 compile-time engine does not: x_backward_kernel
// takes 176 VGPRs there, and the values the loop keeps live pushed the kernel
// into scratch (128 B per lane). Its batches run one single-band launch per
// band, in order on the stream.
template <class Eng>
struct DensityBandLoop {
  static constexpr bool value = true;
};
template <int S, bool LF, bool TwPre>
struct DensityBandLoop<CtEng<float, 1024, S, LF, TwPre>> {
  static constexpr bool value = false;
};

// rho[i] += w |space[i]|^2 in one pass over the space domain (the composed
// density path: R2C transforms and long x lines): E = cx<T> or T.
template <typename E, typename T>
__global__ void __launch_bounds__(256)
    space_density_kernel(const E* __restrict__ space, T* __restrict__ density, T w, long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    T s2;
    if constexpr (std::is_same<E, T>::value) {
      const T s = ld_stream_real(space + i);
      s2 = s * s;
    } else {
      s2 = norm2(ld_stream(space + i));
    }
    st_stream_real(density + i, fma(w, s2, ld_stream_real(density + i)));
  }
}

// ------------------------------------------------------------ spinor operators
// Two-component spinors (up, down): the 2x2 Hermitian local potential
// {v_uu, v_dd, v_ud = v_ud_re + i v_ud_im, v_du = conj(v_ud)} and the spin
// density matrix {n_uu, n_dd, n_ud = up conj(down)}. The x stages keep the
// rows of both components of a tile in LDS at once: region 0 (up) at the start
// of the workgroup's LDS, region 1 (down) `region1` elements behind it, which
// is the engine's whole line LDS (both halves of a ping-pong plan, both
// buffers of Bluestein) rounded up to 16 bytes; the x -> column table follows
// region 1. A workgroup's LDS limit and the bytes of a launch:
constexpr std::size_t kSpinorLdsLimit = 160 * 1024;
inline std::size_t spinor_region_bytes(std::size_t engineBytes) { return (engineBytes + 15) / 16 * 16; }
inline std::size_t spinor_lds_bytes(std::size_t engineBytes, int n) {
  return 2 * spinor_region_bytes(engineBytes) + static_cast<std::size_t>(n) * sizeof(int) + 16;
}
// Compile-time engines that can never fit twice are not instantiated (their
// plans run composed): the 1024-long shapes of both precisions.
template <class Eng>
struct SpinorFits {
  static constexpr bool value = true;
};
template <typename T, int N, int S, bool LF, bool TwPre>
struct SpinorFits<CtEng<T, N, S, LF, TwPre>> {
  static constexpr bool value =
      2 * ((CtEng<T, N, S, LF, TwPre>::F::lds_bytes() + 15) / 16 * 16) + std::size_t(N) * sizeof(int) + 16 <=
      kSpinorLdsLimit;
};

// Kernel arguments, by value: the intermediates of the spinors' members and
// the four real arrays [localZ][Y][X] (potential, read; density, updated).
template <typename T>
struct SpinorApplyArgs {
  cx<T>* up[kMaxSpinors];
  cx<T>* dn[kMaxSpinors];
  const T* v[4];  // v_uu, v_dd, v_ud_re, v_ud_im
};
template <typename T>
struct SpinorDensityArgs {
  const cx<T>* up[kMaxSpinors];
  const cx<T>* dn[kMaxSpinors];
  T w[kMaxSpinors];
  T* n[4];  // n_uu, n_dd, n_ud_re, n_ud_im
  int count;
};

// (u, d) -> (v_uu u + v_ud d, conj(v_ud) u + v_dd d), fixed operation order
template <typename T>
__device__ __forceinline__ void spinor_mix(cx<T>& u, cx<T>& d, T vuu, T vdd, T vre, T vim) {
  const cx<T> ou = mk<T>(fma(vuu, u.x, fma(vre, d.x, -(vim * d.y))), fma(vuu, u.y, fma(vre, d.y, vim * d.x)));
  const cx<T> od = mk<T>(fma(vdd, d.x, fma(vre, u.x, vim * u.y)), fma(vdd, d.y, fma(vre, u.y, -(vim * u.x))));
  u = ou;
  d = od;
}

// The 2x2 mix of both regions for idx in [0, total): lanes walk the rows
// contiguously as in scale_rows, so the loads of the four potential arrays
// coalesce; kApplyUnroll loads per array are in flight per lane. No LDS race:
// lane idx reads src(idx) of region 0 and of region 1 and writes dst(idx) of
// both, and no other lane touches those four slots: src = the inverse engine's
// out_at and dst = the forward engine's in_at are, inside a region, either the
// same slot (compile-time engines, in-place run-time plans, Bluestein) or
// slots of the region's two disjoint halves (ping-pong run-time plans with an
// odd pass count: every read in the second half, every write in the first),
// and region 1 begins behind the whole of region 0, second half included.
// Stream: the potential is read once (non-temporal); plain loads when the
// spinors of a batch share it.
template <bool Stream, typename T, class Src, class Dst>
__device__ __forceinline__ void spinor_mix_rows(cx<T>* ldsU, cx<T>* ldsD, const T* __restrict__ vuu,
                                                const T* __restrict__ vdd, const T* __restrict__ vre,
                                                const T* __restrict__ vim, int total, Src src, Dst dst) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kApplyUnroll) {
    T w[4][kApplyUnroll];
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        if constexpr (Stream) {
          w[0][u] = ld_stream_real(vuu + idx);
          w[1][u] = ld_stream_real(vdd + idx);
          w[2][u] = ld_stream_real(vre + idx);
          w[3][u] = ld_stream_real(vim + idx);
        } else {
          w[0][u] = vuu[idx];
          w[1][u] = vdd[idx];
          w[2][u] = vre[idx];
          w[3][u] = vim[idx];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const int si = src(idx), di = dst(idx);
        cx<T> pu = ldsU[si], pd = ldsD[si];
        spinor_mix(pu, pd, w[0][u], w[1][u], w[2][u], w[3][u]);
        ldsU[di] = pu;
        ldsD[di] = pd;
      }
    }
  }
}

// Fused spinor local-operator x stage (C2C), in place on the two intermediates
// of spinor blockIdx.z. A workgroup owns the tile of x_apply_kernel (plane z,
// rows y0..y0+B, every column) of BOTH components. In-place invariant: the
// first passes of both inverse FFTs have read every element of both tiles
// before either forward FFT stores any (the mix and its barriers lie in
// between), and no other workgroup touches either tile; so out == in per
// member is safe, and so is any order of the members' tiles in memory. The
// component loops are not unrolled: one inlined copy of each FFT, with the
// per-element arguments and the twiddle table pinned anew per component (as
// loop invariants their column offsets would stay live across the loop, see
// x_density_kernel).
template <class Eng, class Fwd, typename T, bool StreamV>
__global__ void __launch_bounds__(Eng::kBlock)
    x_spinor_apply_kernel(Eng eng, Fwd fwd, XArgs a, SpinorApplyArgs<T> sp, int region1,
                          const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  const int r1 = pin_uniform(region1);
  int* xCol = reinterpret_cast<int*>(lds + 2 * r1);
  build_xcol(a, xCol, n);
  const int yl = min(B, a.Y - y0);
  const int s = blockIdx.z;
  const long long tileOff = static_cast<long long>(zl) * a.interZStride + y0;
#pragma unroll 1
  for (int c = 0; c < 2; ++c) {
    // per-element arguments pinned in scalar registers (see x_backward_kernel)
    const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
    const int dense = pin_uniform(x_dense(a) ? 1 : 0);
    const cx<T>* twC = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(tw)));
    const cx<T>* tile = (c ? sp.dn[s] : sp.up[s]) + tileOff;
    auto load = [&](int b, int pos) -> cx<T> {
      if (b >= yl) return czero<T>();
      const int col = dense ? (pos < nFreq ? pos : -1) : xCol[pos];
      return col < 0 ? czero<T>() : ld_inter(&tile[col * rowStride + b]);
    };
    eng.global_to_lds(lds + c * r1, twC, load);  // rows at out_at(b, x); ends with a barrier
  }
  const long long vOff = (static_cast<long long>(zl) * a.Y + y0) * n;
  spinor_mix_rows<StreamV>(lds, lds + r1, sp.v[0] + vOff, sp.v[1] + vOff, sp.v[2] + vOff, sp.v[3] + vOff,
                           yl * n, [&](int idx) {
    const int b = idx / n;
    return eng.out_at(b, idx - b * n);
  }, [&](int idx) {
    const int b = idx / n;
    return fwd.in_at(b, idx - b * n);
  });
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < 2; ++c) {
    const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
    const int dense = pin_uniform(x_dense(a) ? 1 : 0);
    const cx<T>* twC = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(tw)));
    cx<T>* tile = (c ? sp.dn[s] : sp.up[s]) + tileOff;
    auto store = [&](int b, int pos, cx<T> v) {
      const int col = dense ? (pos < nFreq ? pos : -1) : xCol[pos];
      if (col >= 0 && b < yl) st_inter(&tile[col * rowStride + b], v);
    };
    fwd.lds_to_global(lds + c * r1, twC, store);
  }
}

// n_uu += w |u|^2, n_dd += w |d|^2, n_ud += w u conj(d) for one element
template <typename T>
__device__ __forceinline__ void spin_density_add(T w, cx<T> u, cx<T> d, T& nuu, T& ndd, T& nre, T& nim) {
  nuu = fma(w, norm2(u), nuu);
  ndd = fma(w, norm2(d), ndd);
  nre = fma(w, fma(u.x, d.x, u.y * d.y), nre);
  nim = fma(w, fma(u.y, d.x, -(u.x * d.y)), nim);
}

// The four-array update for idx in [0, total), rows walked contiguously as in
// density_rows. x_spinor_density_kernel carries four values per element where
// x_density_kernel carries one, so the unroll is kDensityUnroll / 2: eight
// loads in flight per lane before the first dependent store, twice those of
// density_rows, at twice its registers (an unroll of 4 would hold sixteen
// values, the doubling that spilled x_density_kernel at N = 1024).
constexpr int kSpinDensityUnroll = 2;
template <bool Stream, typename T, class Src>
__device__ __forceinline__ void spin_density_rows(const cx<T>* ldsU, const cx<T>* ldsD, T* __restrict__ nuu,
                                                  T* __restrict__ ndd, T* __restrict__ nre,
                                                  T* __restrict__ nim, T w, int total, Src src) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kSpinDensityUnroll) {
    T r[4][kSpinDensityUnroll];
#pragma unroll
    for (int u = 0; u < kSpinDensityUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        if constexpr (Stream) {
          r[0][u] = ld_stream_real(nuu + idx);
          r[1][u] = ld_stream_real(ndd + idx);
          r[2][u] = ld_stream_real(nre + idx);
          r[3][u] = ld_stream_real(nim + idx);
        } else {
          r[0][u] = nuu[idx];
          r[1][u] = ndd[idx];
          r[2][u] = nre[idx];
          r[3][u] = nim[idx];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kSpinDensityUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const int si = src(idx);
        spin_density_add(w, ldsU[si], ldsD[si], r[0][u], r[1][u], r[2][u], r[3][u]);
        if constexpr (Stream) {
          st_stream_real(nuu + idx, r[0][u]);
          st_stream_real(ndd + idx, r[1][u]);
          st_stream_real(nre + idx, r[2][u]);
          st_stream_real(nim + idx, r[3][u]);
        } else {
          nuu[idx] = r[0][u];
          ndd[idx] = r[1][u];
          nre[idx] = r[2][u];
          nim[idx] = r[3][u];
        }
      }
    }
  }
}

// Registers a lane may spend on the accumulators of the register path below
// (32-bit registers: four values per element, two registers per fp64 value):
// an eighth of the lane's register file at the kernel's launch bound, 64 for
// workgroups of up to 256 threads (8 elements per lane in fp64, 16 in fp32),
// 32 for the wider shapes, whose waves share a SIMD's registers two by two.
// With 64 everywhere the fp32 N = 512 and N = 360 shapes (512 and 384
// threads, 15-16 elements per lane) spilled 84 B per lane.
template <class Eng>
constexpr int spin_density_acc_regs() {
  return Eng::kBlock <= kMaxThreads ? 64 : 32;
}

// Fused spin-density x stage (C2C). Tile ownership of x_density_kernel: the
// workgroup owns plane z, rows y0..y0+B of the four density arrays, so no
// atomics; it loops over the sp.count spinors of the launch with both
// components' rows in LDS (regions 0 and 1), and lane idx updates the same
// elements for every spinor, in spinor order: the sum order is fixed. Full
// tiles of compile-time engines whose accumulators fit spin_density_acc_regs sum
// in registers and touch the arrays once; otherwise every spinor's update goes
// to the arrays, ordered by the lane's own program order. Stream: the cache
// policy of the array accesses of a single-spinor launch.
template <class Eng, typename T, bool Stream>
__global__ void __launch_bounds__(Eng::kBlock)
    x_spinor_density_kernel(Eng eng, XArgs a, SpinorDensityArgs<T> sp, int region1,
                            const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  const int r1 = pin_uniform(region1);
  int* xCol = reinterpret_cast<int*>(lds + 2 * r1);
  build_xcol(a, xCol, n);
  const int yl = min(B, a.Y - y0);
  const long long tileOff = static_cast<long long>(zl) * a.interZStride + y0;
  const long long nOff = (static_cast<long long>(zl) * a.Y + y0) * n;
  T* nuu = sp.n[0] + nOff;
  T* ndd = sp.n[1] + nOff;
  T* nre = sp.n[2] + nOff;
  T* nim = sp.n[3] + nOff;
  // inverse x FFTs of spinor m's two tiles: rows at out_at(b, x) of regions 0 and 1
  auto spinor_fft = [&](int m) {
    if (m > 0) __syncthreads();  // the previous spinor's rows have been read
#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
      // pinned anew per component and spinor (see x_density_kernel's band loop)
      const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
      const int dense = pin_uniform(x_dense(a) ? 1 : 0);
      const cx<T>* twC = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(tw)));
      const cx<T>* tile = (c ? sp.dn[m] : sp.up[m]) + tileOff;
      auto load = [&](int b, int pos) -> cx<T> {
        if (b >= yl) return czero<T>();
        const int col = dense ? (pos < nFreq ? pos : -1) : xCol[pos];
        return col < 0 ? czero<T>() : ld_inter(&tile[col * rowStride + b]);
      };
      eng.global_to_lds(lds + c * r1, twC, load);  // ends with a barrier
    }
  };
  auto row_at = [&](int idx) {
    const int b = idx / n;
    return eng.out_at(b, idx - b * n);
  };
  const int count = pin_uniform(sp.count);
  if constexpr (!Eng::kBatchedCopy && !Stream) {
    using F = typename Eng::F;
    constexpr bool kEven = (F::B * Eng::kN) % F::NT == 0;
    constexpr int kIters = kEven ? F::B * Eng::kN / F::NT : 1;
    constexpr bool kRegs = kEven && 4 * kIters * static_cast<int>(sizeof(T) / 4) <= spin_density_acc_regs<Eng>();
    if (kRegs && yl == F::B) {
      T acc[4][kIters];
#pragma unroll
      for (int i = 0; i < kIters; ++i) acc[0][i] = acc[1][i] = acc[2][i] = acc[3][i] = T(0);
      for (int m = 0; m < count; ++m) {
        spinor_fft(m);
        const T w = sp.w[m];
#pragma unroll
        for (int i = 0; i < kIters; ++i) {
          const int si = row_at(static_cast<int>(threadIdx.x) + i * F::NT);
          spin_density_add(w, lds[si], lds[r1 + si], acc[0][i], acc[1][i], acc[2][i], acc[3][i]);
        }
      }
      T* arr[4] = {nuu, ndd, nre, nim};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int i = 0; i < kIters; ++i) acc[k][i] += arr[k][static_cast<int>(threadIdx.x) + i * F::NT];
#pragma unroll
        for (int i = 0; i < kIters; ++i) arr[k][static_cast<int>(threadIdx.x) + i * F::NT] = acc[k][i];
      }
      return;
    }
  }
  for (int m = 0; m < count; ++m) {
    spinor_fft(m);
    spin_density_rows<Stream>(lds, lds + r1, nuu, ndd, nre, nim, sp.w[m], yl * n, row_at);
  }
}

// Composed spinor paths, one pass over two complex space domains: the in-place
// 2x2 mix, and the four-array density update.
template <typename T>
__global__ void __launch_bounds__(256)
    space_spinor_mix_kernel(cx<T>* up, cx<T>* dn, const T* vuu, const T* vdd, const T* vre, const T* vim,
                            long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    cx<T> u = ld_stream(up + i), d = ld_stream(dn + i);
    spinor_mix(u, d, vuu[i], vdd[i], vre[i], vim[i]);
    st_stream(up + i, u);
    st_stream(dn + i, d);
  }
}
template <typename T>
__global__ void __launch_bounds__(256)
    space_spin_density_kernel(const cx<T>* __restrict__ up, const cx<T>* __restrict__ dn, T* nuu, T* ndd,
                              T* nre, T* nim, T w, long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    T a = nuu[i], b = ndd[i], c = nre[i], e = nim[i];
    spin_density_add(w, ld_stream(up + i), ld_stream(dn + i), a, b, c, e);
    nuu[i] = a;
    ndd[i] = b;
    nre[i] = c;
    nim[i] = e;
  }
}

// ------------------------------------------------ exchange (Fock) pair operator
// accumulate_fock: acc += w a backward(K forward(conj(a) b)). Fused plans (C2C)
// form the pair density in the forward x stage's row loads and accumulate in
// the backward x stage's copy-out; the space domain is neither written nor read.

// Forward x stage of the pair density: x_forward_kernel (C2C) whose tile rows
// are conj(a) * b of two space-domain arrays. StreamAB: the cache policy of
// their loads (a template parameter: a run-time flag costs registers and can
// lose the hint, profiles/r6/ntmerge). a may be b: both are only read.
template <class Eng, typename T, bool StreamAB>
__device__ __forceinline__ void x_forward_pair_body(const Eng& eng, const XArgs& a, const cx<T>* __restrict__ pa,
                                                    const cx<T>* __restrict__ pb, cx<T>* __restrict__ inter,
                                                    const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, n);
  const int yl = min(B, a.Y - y0);
  cx<T>* dst = inter + static_cast<long long>(zl) * a.interZStride + y0;
  const long long row0 = (static_cast<long long>(zl) * a.Y + y0) * n;
  // arguments of the per-element stores pinned in scalar registers (see x_backward_kernel)
  const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
  const int dense = pin_uniform(x_dense(a) ? 1 : 0);
  auto store = [&](int b, int pos, cx<T> v) {
    const int c = dense ? (pos < nFreq ? pos : -1) : xCol[pos];
    if (c >= 0 && b < yl) st_inter(&dst[c * rowStride + b], v);
  };
  stage_rows(eng, lds, yl, n, PairSrc<T, StreamAB>{{pa + row0, pb + row0}, n});
  eng.lds_to_global(lds, tw, store);
}

template <class Eng, typename T, bool StreamAB>
__global__ void __launch_bounds__(Eng::kBlock)
    x_forward_pair_kernel(Eng eng, XArgs a, const cx<T>* __restrict__ pa, const cx<T>* __restrict__ pb,
                          cx<T>* __restrict__ inter, const cx<T>* __restrict__ tw) {
  x_forward_pair_body<Eng, T, StreamAB>(eng, a, pa, pb, inter, tw);
}

// Per-member arguments of the batched pair launches that BatchPtrs has no room
// for, by value (as DensityWeights): the second input of the forward stage; the
// `a` arrays and weights of the accumulating backward stage.
template <typename T>
struct PairSecond {
  const cx<T>* b[kMaxBatch];
};
template <typename T>
struct FockMembers {
  const cx<T>* a[kMaxBatch];
  T w[kMaxBatch];
};

// Batched launch: blockIdx.z selects the member, whose a is XArgs::batch.in,
// whose b is second.b and whose intermediate is XArgs::batch.out.
template <class Eng, typename T, bool StreamAB>
__global__ void __launch_bounds__(Eng::kBlock)
    x_forward_pair_batch_kernel(Eng eng, XArgs a, PairSecond<T> second, const cx<T>* __restrict__ tw) {
  x_forward_pair_body<Eng, T, StreamAB>(eng, a, static_cast<const cx<T>*>(a.batch.in[blockIdx.z]),
                                        second.b[blockIdx.z], static_cast<cx<T>*>(a.batch.out[blockIdx.z]), tw);
}

// acc[idx] += w a[idx] lds[src(idx)] for idx in [0, total): lanes walk the rows
// contiguously (the order of copy_out). kFockUnroll loads each of a and acc are
// in flight per lane before the first dependent store (acc is not restrict
// against itself: the compiler may not move a load of acc over a store to it).
// The unroll is small for the reason given at density_rows: two complex values
// per element are live on top of the engine's registers.
constexpr int kFockUnroll = 4;
template <bool Stream, typename T, class Src>
__device__ __forceinline__ void fock_rows(const cx<T>* lds, const cx<T>* __restrict__ pa, cx<T>* __restrict__ acc,
                                          T w, int total, Src src) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kFockUnroll) {
    cx<T> av[kFockUnroll], r[kFockUnroll];
#pragma unroll
    for (int u = 0; u < kFockUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        if constexpr (Stream) {
          av[u] = ld_stream(pa + idx);
          r[u] = ld_stream(acc + idx);
        } else {
          av[u] = pa[idx];
          r[u] = acc[idx];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kFockUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const cx<T> t = scale(av[u], w);
        const cx<T> v = lds[src(idx)];
        const cx<T> o = mk<T>(fma(t.x, v.x, fma(-t.y, v.y, r[u].x)), fma(t.x, v.y, fma(t.y, v.x, r[u].y)));
        if constexpr (Stream) st_stream(acc + idx, o);
        else acc[idx] = o;
      }
    }
  }
}

// Backward x stage of the pair operator: the front half of x_backward_kernel
// (C2C: same tile, column lookup and engine), then acc += w a u on the
// workgroup's rows of acc straight from LDS. A workgroup owns its tile's rows of
// acc, so the update needs no atomics. StreamAcc: cache policy of a and acc.
template <class Eng, typename T, bool StreamAcc>
__global__ void __launch_bounds__(Eng::kBlock)
    x_backward_fock_kernel(Eng eng, XArgs a, const cx<T>* __restrict__ inter, const cx<T>* __restrict__ pa,
                           cx<T>* __restrict__ acc, T w, const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, n);
  const cx<T>* src = inter + static_cast<long long>(zl) * a.interZStride + y0;
  const int yl = min(B, a.Y - y0);
  // per-element arguments pinned in scalar registers (see x_backward_kernel)
  const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
  const int dense = pin_uniform(x_dense(a) ? 1 : 0);
  auto col_of = [&](int x) { return dense ? (x < nFreq ? x : -1) : xCol[x]; };
  auto load = [&](int b, int pos) -> cx<T> {
    if (b >= yl) return czero<T>();
    const int c = col_of(pos);
    return c < 0 ? czero<T>() : ld_inter(&src[c * rowStride + b]);
  };
  const long long row0 = (static_cast<long long>(zl) * a.Y + y0) * n;
  eng.global_to_lds(lds, tw, load);  // rows at out_at(b, x); ends with a barrier
  fock_rows<StreamAcc>(lds, pa + row0, acc + row0, w, yl * n, [&](int idx) {
    const int b = idx / n;
    return eng.out_at(b, idx - b * n);
  });
}

// The pairs of a batched launch share acc, so they are not spread over
// blockIdx.z: the workgroup that owns a tile loops over the members in order
// (intermediates from XArgs::batch.in, a and weight from `members`), as
// x_density_kernel does over its bands. Lane idx updates the same elements of
// acc for every member, so a member's update is ordered behind the previous
// one's by the lane's own program order: the sum order is fixed, without
// atomics. The members revisit the tile of acc, so its accesses (and those of
// a) take the default cache policy.
template <class Eng, typename T>
__global__ void __launch_bounds__(Eng::kBlock)
    x_backward_fock_batch_kernel(Eng eng, XArgs a, FockMembers<T> members, cx<T>* __restrict__ acc,
                                 const cx<T>* __restrict__ tw) {
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int n = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, n);
  const int yl = min(B, a.Y - y0);
  const long long row0 = (static_cast<long long>(zl) * a.Y + y0) * n;
  for (int m = 0; m < a.batch.count; ++m) {
    // the per-element arguments and the twiddle table are pinned anew for every
    // member: as loop invariants they were hoisted out of the loop and stayed
    // live across it (see x_density_kernel)
    const cx<T>* twM = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(tw)));
    const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
    const int dense = pin_uniform(x_dense(a) ? 1 : 0);
    auto col_of = [&](int x) { return dense ? (x < nFreq ? x : -1) : xCol[x]; };
    const cx<T>* src = static_cast<const cx<T>*>(a.batch.in[m]) + static_cast<long long>(zl) * a.interZStride + y0;
    auto load = [&](int b, int pos) -> cx<T> {
      if (b >= yl) return czero<T>();
      const int c = col_of(pos);
      return c < 0 ? czero<T>() : ld_inter(&src[c * rowStride + b]);
    };
    if (m > 0) __syncthreads();  // the previous member's rows have been read
    eng.global_to_lds(lds, twM, load);  // rows at out_at(b, x); ends with a barrier
    fock_rows<false>(lds, members.a[m] + row0, acc + row0, members.w[m], yl * n, [&](int idx) {
      const int b = idx / n;
      return eng.out_at(b, idx - b * n);
    });
  }
}

// Engines whose batched accumulating x stage keeps the member loop inside the
// workgroup; the others run one single-pair launch per member, in order on the
// stream (the DensityBandLoop pattern). The fp32 N = 1024 compile-time engine
// does not: with the loop its kernel took all 256 VGPRs and 96 B of scratch
// per lane (23 spilled registers).
template <class Eng>
struct FockBandLoop {
  static constexpr bool value = true;
};
template <int S, bool LF, bool TwPre>
struct FockBandLoop<CtEng<float, 1024, S, LF, TwPre>> {
  static constexpr bool value = false;
};

// The composed pair operator's two passes over the space domain (R2C transforms
// and long x lines): E = cx<T> or T (conj is then the identity).
// space[i] = conj(a[i]) * b[i]
template <typename E, typename T>
__global__ void __launch_bounds__(256)
    space_pair_kernel(E* __restrict__ space, const E* pa, const E* pb, long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    if constexpr (std::is_same<E, T>::value)
      st_stream_real(space + i, ld_stream_real(pa + i) * ld_stream_real(pb + i));
    else
      st_stream(space + i, cmulc(ld_stream(pb + i), ld_stream(pa + i)));
  }
}
// acc[i] += w * a[i] * space[i]
template <typename E, typename T>
__global__ void __launch_bounds__(256)
    space_fock_kernel(const E* __restrict__ space, const E* __restrict__ pa, E* __restrict__ acc, T w,
                      long long count) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    if constexpr (std::is_same<E, T>::value) {
      st_stream_real(acc + i, fma(w * ld_stream_real(pa + i), ld_stream_real(space + i), ld_stream_real(acc + i)));
    } else {
      const cx<T> t = scale(ld_stream(pa + i), w);
      const cx<T> v = ld_stream(space + i);
      const cx<T> r = ld_stream(acc + i);
      st_stream(acc + i, mk<T>(fma(t.x, v.x, fma(-t.y, v.y, r.x)), fma(t.x, v.y, fma(t.y, v.x, r.y))));
    }
  }
}

// Packed-real x stage (R2C transforms with even dimX): a real row of length n
// is the complex sequence y[m] = x[2m] + i x[2m+1] of length h = n/2, so one
// half-length FFT plus a twiddle pre-pass (C2R) or post-pass (R2C) replaces the
// hermitian-extended length-n complex FFT: half the butterflies, half the LDS
// traffic, and the real row is read/written as h contiguous complex values.
//   C2R: Z[k] = (X[k] + conj X[h-k]) + i (X[k] - conj X[h-k]) w^k,  y = IDFT_h(Z)
//   R2C: Y = DFT_h(y),  X[k] = (Y[k] + conj Y[h-k])/2 + w^k (Y[k] - conj Y[h-k])/(2i)
// with w = exp(S 2 pi i / n); the imaginary parts of X[0] and X[h] are ignored
// (they cannot contribute to a real signal), as in the complex C2R path.
// first-pass radix of a compile-time engine (0: mixed-radix engines)
template <class F, class = void>
struct FirstRadix {
  static constexpr int value = 0;
};
template <class F>
struct FirstRadix<F, std::void_t<typename F::Sh>> {
  static constexpr int value = F::Sh::R0;
};

template <class Eng, typename T>
__global__ void __launch_bounds__(Eng::kBlock)
    x_backward_c2r_kernel(Eng eng, XArgs a, const cx<T>* __restrict__ inter, T* __restrict__ space,
                          const cx<T>* __restrict__ twh, const cx<T>* __restrict__ twn) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, inter, space);
  const int B = eng.lines();
  const int h = eng.n();
  const long long n = 2 * static_cast<long long>(h);
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  // LDS: FFT lines | X[h] (Nyquist) per line | xCol table
  cx<T>* nyq = reinterpret_cast<cx<T>*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  int* xCol = reinterpret_cast<int*>(nyq + B);
  build_xcol(a, xCol, h + 1);
  const cx<T>* src = inter + static_cast<long long>(zl) * a.interZStride + y0;
  const int yl = min(B, a.Y - y0);
  if constexpr (!Eng::kBatchedCopy) {
    // pre-pass folded into the FFT's first-pass loads: the lane that needs Z[k]
    // loads X[k] and X[h-k] itself (the mirror column is the same workgroup's
    // data, so its second read is served by the caches; plain loads keep it there:
    // streamed loads measured 197.7 -> 239.1 us at 512^3 R2C fp32, profiles/r6/ntmerge/c2r_ab.txt)
    // arguments of the per-element loads pinned in scalar registers (see x_backward_kernel)
    const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
    const int dense = pin_uniform(x_dense(a) ? 1 : 0);
    auto col = [&](int k, int b) -> cx<T> {
      const int c = dense ? (k < nFreq ? k : -1) : xCol[k];
      return (c < 0 || b >= yl) ? czero<T>() : src[c * rowStride + b];
    };
    // twiddle w^k of position k = t + off, off = kk*TP + r*(h/R0): the table
    // entry of t + kk*TP times the compile-time root exp(-i pi r / R0), so a
    // lane loads one entry per kk instead of one per element: 131 -> 115 VGPRs
    // (fp32 h = 256), x backward at 512^3 R2C fp32 259.2 -> 217.9 us, 256^3 R2C
    // fp64 55.5 -> 54.5 us (profiles/r5/ab/c2r_twiddles)
    constexpr int R0 = FirstRadix<typename Eng::F>::value, Q = R0 ? Eng::kN / R0 : 1;
    eng.global_to_lds(lds, twh, [&](int b, int k, int off) -> cx<T> {
      cx<T> xk = col(k, b);
      cx<T> xm = col(h - k, b);
      if (k == 0) {
        xk.y = T(0);
        xm.y = T(0);
      }
      const cx<T> xmc = conj(xm);
      const int r = off / Q;
      cx<T> w = twn[k - r * Q];
      if constexpr (R0 == 16) {
        if (r) w = cmul(w, mk<T>(T(fftc::C32[r & 15]), T(-fftc::S32[r & 15])));
      } else if constexpr (R0 == 8) {
        if (r) w = cmul(w, mk<T>(T(fftc::C16[r & 15]), T(-fftc::S16[r & 15])));
      } else {
        w = twn[k];
      }
      return (xk + xmc) + rot<+1>(twm<+1>(xk - xmc, w));
    });
    cx<T>* out = reinterpret_cast<cx<T>*>(space + (static_cast<long long>(zl) * a.Y + y0) * n);
    copy_out<Eng>(lds, yl * h, [&](int idx) {
      const int b = idx / h;
      return eng.out_at(b, idx - b * h);
    }, [&](int idx, cx<T> v) { st_stream(&out[idx], v); });
    return;
  }
  // columns X[0..h] of the block's rows, each element loaded once (lanes run
  // over rows: contiguous column segments)
  gather_to_lds(lds, h * B, [&](int idx) -> cx<T> {
    const int k = idx / B, b = idx - k * B;
    const int c = xcol_of(a, xCol, k);
    return (c < 0 || b >= yl) ? czero<T>() : ld_inter(&src[inter_row(a, c) + b]);
  }, [&](int idx) {
    const int k = idx / B;
    return eng.in_at(idx - k * B, k);
  });
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int c = xcol_of(a, xCol, h);
    nyq[b] = (c < 0 || b >= yl) ? czero<T>() : ld_inter(&src[inter_row(a, c) + b]);
  }
  __syncthreads();
  // pre-pass in place, pairs (k, h-k): Z[k] = (X[k] + conj X[h-k]) + i (X[k] - conj X[h-k]) w^k
  for (int idx = threadIdx.x; idx < B * (h / 2 + 1); idx += blockDim.x) {
    const int k = idx / B, b = idx - k * B;
    const int m = h - k;
    cx<T> xk = lds[eng.in_at(b, k)];
    cx<T> xm = m == h ? nyq[b] : lds[eng.in_at(b, m)];
    if (k == 0) {
      xk.y = T(0);
      xm.y = T(0);
    }
    const cx<T> xmc = conj(xm), xkc = conj(xk);
    lds[eng.in_at(b, k)] = (xk + xmc) + rot<+1>(twm<+1>(xk - xmc, twn[k]));
    if (m != k && m < h) lds[eng.in_at(b, m)] = (xm + xkc) + rot<+1>(twm<+1>(xm - xkc, twn[m]));
  }
  __syncthreads();
  eng.lds_to_lds(lds, twh);
  // the yl rows are contiguous in the space domain: one coalesced copy-out
  cx<T>* out = reinterpret_cast<cx<T>*>(space + (static_cast<long long>(zl) * a.Y + y0) * n);
  copy_out<Eng>(lds, yl * h, [&](int idx) {
    const int b = idx / h;
    return eng.out_at(b, idx - b * h);
  }, [&](int idx, cx<T> v) { st_stream(&out[idx], v); });
}

template <class Eng, typename T>
__global__ void __launch_bounds__(Eng::kBlock)
    x_forward_r2c_kernel(Eng eng, XArgs a, const T* __restrict__ space, cx<T>* __restrict__ inter,
                         const cx<T>* __restrict__ twh, const cx<T>* __restrict__ twn) {
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, space, inter);
  const int B = eng.lines();
  const int h = eng.n();
  const long long n = 2 * static_cast<long long>(h);
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, h + 1);
  const int yl = min(B, a.Y - y0);
  const cx<T>* row0 = reinterpret_cast<const cx<T>*>(space + (static_cast<long long>(zl) * a.Y + y0) * n);
  auto rowLoad = [&](int b, int m) -> cx<T> {
    return b >= yl ? czero<T>() : ld_stream(row0 + static_cast<long long>(b) * h + m);
  };
  if constexpr (!Eng::kBatchedCopy && !Eng::kLineFast) {
    // row-mapped engine (launch_x_forward): a line's lanes are adjacent, so the
    // first pass loads the real rows straight from global memory
    eng.global_to_lds(lds, twh, rowLoad);
  } else {
    stage_rows(eng, lds, yl, h, RowSrc<cx<T>>{row0, h});
    eng.lds_to_lds(lds, twh);
  }
  cx<T>* dst = inter + static_cast<long long>(zl) * a.interZStride + y0;
  // post pass over the pairs (k, h - k), k <= h/2: both outputs need the same
  // two LDS values, and w^(h-k) = -conj(w^k) (w = exp(-2 pi i / n), n = 2h), so
  // a pair costs two LDS reads and one twiddle load instead of four and two
  // (512^3 R2C fp32 x forward 224-226 -> 214-216 us, 256^3 R2C fp64 55 -> 53 us,
  // profiles/r5/ab/r2cpair). Lanes run over rows first, so the column stores are
  // contiguous.
  for (int idx = threadIdx.x; idx < B * (h / 2 + 1); idx += blockDim.x) {
    const int b = idx % B, k = idx / B, m = h - k;
    if (b >= yl) continue;
    const int ck = xcol_of(a, xCol, k), cm = xcol_of(a, xCol, m);
    if (ck < 0 && cm < 0) continue;
    const cx<T> A = lds[eng.out_at(b, k == h ? 0 : k)];
    const cx<T> Bv = lds[eng.out_at(b, m == h ? 0 : m)];
    const cx<T> wk = twn[k];
    if (ck >= 0) {
      const cx<T> ym = conj(Bv);
      const cx<T> e = scale(A + ym, T(0.5));
      const cx<T> o = scale(rot<-1>(A - ym), T(0.5));
      st_inter(&dst[inter_row(a, ck) + b], e + twm<-1>(o, wk));
    }
    if (cm >= 0 && m != k) {
      const cx<T> ym = conj(A);
      const cx<T> e = scale(Bv + ym, T(0.5));
      const cx<T> o = scale(rot<-1>(Bv - ym), T(0.5));
      st_inter(&dst[inter_row(a, cm) + b], e + twm<-1>(o, mk<T>(-wk.x, wk.y)));
    }
  }
}

// ------------------------------------------- fused operators on packed-real rows
// apply_local and accumulate_density of R2C transforms whose half-length h =
// dimX / 2 has a compile-time engine: the x stages below work on the rows y[m] =
// s[2m] + i s[2m+1] of the packed-real stage in LDS, and the real space domain
// is neither read nor written. Compile-time engines only (the run-time and
// Bluestein half-lengths stay composed): the C2R pre-pass rides on the first
// pass's loads, as in x_backward_c2r_kernel.
//
// Engines whose fused packed-real kernels are not built; their plans run
// composed (x_r2c_fused_fits).
template <class Eng>
struct R2cFuseFits {
  static constexpr bool value = !Eng::kBatchedCopy;
};

// Inverse half-length FFT of the tile's packed-real rows with the C2R pre-pass
// folded into the first-pass loads (the body of x_backward_c2r_kernel's
// compile-time path, kept apart from it so that kernel's code is untouched):
// Z[k] from X[k] and X[h-k], imaginary parts of X[0] and X[h] dropped, columns
// without sticks read as zero. Row b ends at eng.out_at(b, m); ends with a
// barrier. Every global load of the tile `src` happens here.
template <class Eng, typename T>
__device__ __forceinline__ void c2r_rows_to_lds(Eng eng, cx<T>* lds, const XArgs& a, const int* xCol,
                                                const cx<T>* src, int yl, const cx<T>* __restrict__ twh,
                                                const cx<T>* __restrict__ twn) {
  const int h = eng.n();
  // arguments of the per-element loads pinned in scalar registers (see x_backward_kernel)
  const int rowStride = pin_uniform(static_cast<int>(a.interStride)), nFreq = pin_uniform(a.nFreq);
  const int dense = pin_uniform(x_dense(a) ? 1 : 0);
  auto col = [&](int k, int b) -> cx<T> {
    const int c = dense ? (k < nFreq ? k : -1) : xCol[k];
    return (c < 0 || b >= yl) ? czero<T>() : src[c * rowStride + b];
  };
  // (the twiddle of position k from one table entry per kk: see x_backward_c2r_kernel)
  constexpr int R0 = FirstRadix<typename Eng::F>::value, Q = R0 ? Eng::kN / R0 : 1;
  eng.global_to_lds(lds, twh, [&](int b, int k, int off) -> cx<T> {
    cx<T> xk = col(k, b);
    cx<T> xm = col(h - k, b);
    if (k == 0) {
      xk.y = T(0);
      xm.y = T(0);
    }
    const cx<T> xmc = conj(xm);
    const int r = off / Q;
    cx<T> w = twn[k - r * Q];
    if constexpr (R0 == 16) {
      if (r) w = cmul(w, mk<T>(T(fftc::C32[r & 15]), T(-fftc::S32[r & 15])));
    } else if constexpr (R0 == 8) {
      if (r) w = cmul(w, mk<T>(T(fftc::C16[r & 15]), T(-fftc::S16[r & 15])));
    } else {
      w = twn[k];
    }
    return (xk + xmc) + rot<+1>(twm<+1>(xk - xmc, w));
  });
}

// lds[dst(idx)] = {lds[src(idx)].x * v[idx].x, lds[src(idx)].y * v[idx].y} for
// idx in [0, total): scale_rows on packed-real rows, the potential row read as
// pairs (V[2m], V[2m+1]). Same walk, same kApplyUnroll loads in flight, and the
// same reason for no LDS race: lane idx reads src(idx) and writes dst(idx), and
// the kernel passes the inverse engine's out_at and its forward twin's in_at,
// which are the same slot (compile-time engines on one layout, the
// static_assert of forward_twin). `v` must be aligned to one pair.
template <bool Stream, typename T, class Src, class Dst>
__device__ __forceinline__ void scale_row_pairs(cx<T>* lds, const cx<T>* __restrict__ v, int total, Src src,
                                                Dst dst) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kApplyUnroll) {
    cx<T> w[kApplyUnroll];
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        if constexpr (Stream) w[u] = ld_stream(v + idx);
        else w[u] = v[idx];
      }
    }
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const cx<T> y = lds[src(idx)];
        lds[dst(idx)] = mk<T>(y.x * w[u].x, y.y * w[u].y);
      }
    }
  }
}

// Fused local-operator x stage (R2C, packed-real), in place on the [z][column][y]
// intermediate: a workgroup owns the tile of x_backward_c2r_kernel (plane z,
// rows y0..y0+B, columns 0..h).
//  (a) C2R pre-pass in the first-pass loads + inverse half-length FFT,
//  (b) y.x *= V[2m], y.y *= V[2m+1] in LDS,
//  (c) forward half-length FFT on forward_twin(eng), LDS to LDS,
//  (d) the post pass of x_forward_r2c_kernel over the pairs (k, h-k), Nyquist
//      column included, columns without sticks skipped.
// Invariant that makes the in-place update safe: every global load of the tile
// happens in (a), every store in (d), the barriers of (a), (b) and (c) lie
// between them, and no other workgroup touches the tile. (b) has no LDS race:
// see scale_row_pairs. LDS: FFT lines | one unused element per line (the
// Nyquist slot of the C2R launch, whose LDS and grid this launch takes) | xCol.
template <class Eng, class Fwd, typename T, bool StreamV>
__global__ void __launch_bounds__(Eng::kBlock)
    x_apply_r2c_kernel(Eng eng, Fwd fwd, XArgs a, const T* __restrict__ potential, cx<T>* inter,
                       const cx<T>* __restrict__ twh, const cx<T>* __restrict__ twn) {
  static_assert(!Eng::kBatchedCopy, "x apply r2c: compile-time engines only");
  SPFFT_LDS_DECL(T);
  SPFFT_BATCH_SELECT(a, potential, inter);
  const int B = eng.lines();
  const int h = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<cx<T>*>(reinterpret_cast<char*>(lds) + eng.lds_bytes()) + B);
  build_xcol(a, xCol, h + 1);
  cx<T>* tile = inter + static_cast<long long>(zl) * a.interZStride + y0;
  const int yl = min(B, a.Y - y0);
  c2r_rows_to_lds(eng, lds, a, xCol, tile, yl, twh, twn);  // (a); ends with a barrier
  const cx<T>* v = reinterpret_cast<const cx<T>*>(potential + (static_cast<long long>(zl) * a.Y + y0) * 2 * h);
  scale_row_pairs<StreamV>(lds, v, yl * h, [&](int idx) {
    const int b = idx / h;
    return eng.out_at(b, idx - b * h);
  }, [&](int idx) {
    const int b = idx / h;
    return fwd.in_at(b, idx - b * h);
  });
  __syncthreads();
  fwd.lds_to_lds(lds, twh);  // (c); ends with a barrier
  // (d): both outputs of a pair need the same two LDS values, and w^(h-k) =
  // -conj(w^k); lanes run over rows first, so the column stores are contiguous
  for (int idx = threadIdx.x; idx < B * (h / 2 + 1); idx += blockDim.x) {
    const int b = idx % B, k = idx / B, m = h - k;
    if (b >= yl) continue;
    const int ck = xcol_of(a, xCol, k), cm = xcol_of(a, xCol, m);
    if (ck < 0 && cm < 0) continue;
    const cx<T> A = lds[fwd.out_at(b, k == h ? 0 : k)];
    const cx<T> Bv = lds[fwd.out_at(b, m == h ? 0 : m)];
    const cx<T> wk = twn[k];
    if (ck >= 0) {
      const cx<T> ym = conj(Bv);
      const cx<T> e = scale(A + ym, T(0.5));
      const cx<T> o = scale(rot<-1>(A - ym), T(0.5));
      st_inter(&tile[inter_row(a, ck) + b], e + twm<-1>(o, wk));
    }
    if (cm >= 0 && m != k) {
      const cx<T> ym = conj(A);
      const cx<T> e = scale(Bv + ym, T(0.5));
      const cx<T> o = scale(rot<-1>(Bv - ym), T(0.5));
      st_inter(&tile[inter_row(a, cm) + b], e + twm<-1>(o, mk<T>(-wk.x, wk.y)));
    }
  }
}

// Engines whose batched packed-real density launch sums the bands of a full tile
// in registers. A lane holds twice the values of x_density_kernel's sum (pairs),
// which spilled on the fp64 h = 1024 shape (328 B per lane) and the fp32 h = 360
// one (204 B): those update rho band by band, like partial tiles.
template <class Eng>
struct R2cDensityRegSum {
  static constexpr bool value = true;
};
template <int S, bool LF, bool TwPre>
struct R2cDensityRegSum<CtEng<double, 1024, S, LF, TwPre>> {
  static constexpr bool value = false;
};
template <int S, bool LF, bool TwPre>
struct R2cDensityRegSum<CtEng<float, 360, S, LF, TwPre>> {
  static constexpr bool value = false;
};
// Engines whose batched packed-real density launch keeps the band loop inside the
// workgroup (DensityBandLoop of the C2C stage). The fp32 h = 512 and h = 1024
// shapes do not: the values the loop keeps live spilled with and without the
// register sum (84 B and 292 B per lane without it). Their batches run one
// single-band launch per band, in order on the stream.
template <class Eng>
struct R2cDensityBandLoop {
  static constexpr bool value = true;
};
template <int S, bool LF, bool TwPre>
struct R2cDensityBandLoop<CtEng<float, 512, S, LF, TwPre>> {
  static constexpr bool value = false;
};
template <int S, bool LF, bool TwPre>
struct R2cDensityBandLoop<CtEng<float, 1024, S, LF, TwPre>> {
  static constexpr bool value = false;
};

// rho pair idx += w * {lds[src(idx)].x^2, lds[src(idx)].y^2} for idx in
// [0, total): density_rows on packed-real rows (y.x = s[2m], y.y = s[2m+1]),
// rho read and written as pairs. `rho` must be aligned to one pair.
template <bool Stream, typename T, class Src>
__device__ __forceinline__ void density_row_pairs(const cx<T>* lds, cx<T>* __restrict__ rho, T w, int total,
                                                  Src src) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kDensityUnroll) {
    cx<T> r[kDensityUnroll];
#pragma unroll
    for (int u = 0; u < kDensityUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        if constexpr (Stream) r[u] = ld_stream(rho + idx);
        else r[u] = rho[idx];
      }
    }
#pragma unroll
    for (int u = 0; u < kDensityUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const cx<T> y = lds[src(idx)];
        const cx<T> v = mk<T>(fma(w, y.x * y.x, r[u].x), fma(w, y.y * y.y, r[u].y));
        if constexpr (Stream) st_stream(rho + idx, v);
        else rho[idx] = v;
      }
    }
  }
}

// Fused density x stage (R2C, packed-real): step (a) of x_apply_r2c_kernel, then
// rho[2m] += w y.x^2, rho[2m+1] += w y.y^2 on the workgroup's rows of rho. Tile
// ownership, the band loop, the fixed sum order and the in-register sum of full
// tiles are those of x_density_kernel; LDS and grid those of the C2R launch.
template <class Eng, typename T, bool StreamRho, bool Batched>
__global__ void __launch_bounds__(Eng::kBlock)
    x_density_r2c_kernel(Eng eng, XArgs a, const cx<T>* __restrict__ inter, T* __restrict__ density,
                         DensityWeights<T> weights, const cx<T>* __restrict__ twh,
                         const cx<T>* __restrict__ twn) {
  static_assert(!Eng::kBatchedCopy, "x density r2c: compile-time engines only");
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int h = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<cx<T>*>(reinterpret_cast<char*>(lds) + eng.lds_bytes()) + B);
  build_xcol(a, xCol, h + 1);
  const int yl = min(B, a.Y - y0);
  cx<T>* rho = reinterpret_cast<cx<T>*>(density + (static_cast<long long>(zl) * a.Y + y0) * 2 * h);
  auto fft = [&](const cx<T>* interM, const cx<T>* twhM, const cx<T>* twnM) {
    c2r_rows_to_lds(eng, lds, a, xCol, interM + static_cast<long long>(zl) * a.interZStride + y0, yl, twhM, twnM);
  };
  auto row_at = [&](int idx) {
    const int b = idx / h;
    return eng.out_at(b, idx - b * h);
  };
  if constexpr (!Batched) {
    fft(inter, twh, twn);
    density_row_pairs<StreamRho>(lds, rho, weights.w[0], yl * h, row_at);
  } else {
    // the twiddle tables are pinned anew for every band (see x_density_kernel)
    auto band_fft = [&](int m) {
      const cx<T>* twhM = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(twh)));
      const cx<T>* twnM = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(twn)));
      if (m > 0) __syncthreads();  // the previous band's rows have been read
      fft(static_cast<const cx<T>*>(a.batch.in[m]), twhM, twnM);
    };
    using F = typename Eng::F;
    constexpr bool kEven = R2cDensityRegSum<Eng>::value && (F::B * Eng::kN) % F::NT == 0;
    if (kEven && yl == F::B) {
      constexpr int kIters = kEven ? F::B * Eng::kN / F::NT : 1;
      cx<T> acc[kIters];
#pragma unroll
      for (int i = 0; i < kIters; ++i) acc[i] = czero<T>();
      for (int m = 0; m < a.batch.count; ++m) {
        band_fft(m);
        const T w = weights.w[m];
#pragma unroll
        for (int i = 0; i < kIters; ++i) {
          const cx<T> y = lds[row_at(static_cast<int>(threadIdx.x) + i * F::NT)];
          acc[i] = mk<T>(fma(w, y.x * y.x, acc[i].x), fma(w, y.y * y.y, acc[i].y));
        }
      }
#pragma unroll
      for (int i = 0; i < kIters; ++i) acc[i] = acc[i] + rho[static_cast<int>(threadIdx.x) + i * F::NT];
#pragma unroll
      for (int i = 0; i < kIters; ++i) rho[static_cast<int>(threadIdx.x) + i * F::NT] = acc[i];
      return;
    }
    for (int m = 0; m < a.batch.count; ++m) {
      band_fft(m);
      density_row_pairs<StreamRho>(lds, rho, weights.w[m], yl * h, row_at);
    }
  }
}

// ------------------------------------- pair operator (Fock) on packed-real rows
// accumulate_fock of R2C transforms whose half-length h = dimX / 2 has a
// compile-time engine: a, b and acc are real fields, the pair density a b is
// formed as packed rows in the forward x stage's row loads, and the accumulating
// backward x stage updates pairs of acc straight from LDS. The real space domain
// is neither written nor read. The kernels are built for the engines of
// R2cFuseFits (x_r2c_fock_fits asks it for both directions' engines): no
// single-pair kernel of a compile-time engine spilled, so none is excluded.

// Forward x stage of the pair density (R2C, packed-real): x_forward_r2c_kernel
// whose packed rows are y[m] = a[2m] b[2m] + i a[2m+1] b[2m+1] of two real
// space-domain arrays (PairRealSrc); the forward half-length FFT and the post
// pass over the pairs (k, h - k) are that kernel's. StreamAB: the cache policy
// of the loads of a and b. a may be b: both are only read.
template <class Eng, typename T, bool StreamAB>
__device__ __forceinline__ void x_forward_pair_r2c_body(const Eng& eng, const XArgs& a, const T* __restrict__ pa,
                                                        const T* __restrict__ pb, cx<T>* __restrict__ inter,
                                                        const cx<T>* __restrict__ twh,
                                                        const cx<T>* __restrict__ twn) {
  static_assert(!Eng::kBatchedCopy, "x forward pair r2c: compile-time engines only");
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int h = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + eng.lds_bytes());
  build_xcol(a, xCol, h + 1);
  const int yl = min(B, a.Y - y0);
  const long long off = (static_cast<long long>(zl) * a.Y + y0) * h;  // in pairs
  const PairRealPtr<T, StreamAB> row0{reinterpret_cast<const cx<T>*>(pa) + off,
                                      reinterpret_cast<const cx<T>*>(pb) + off};
  if constexpr (!Eng::kLineFast) {
    // row-mapped engine: the first pass loads the product rows straight from global memory
    eng.global_to_lds(lds, twh, [&](int b, int m) -> cx<T> {
      return b >= yl ? czero<T>() : row_elem<T>(row0 + (static_cast<long long>(b) * h + m));
    });
  } else {
    stage_rows(eng, lds, yl, h, PairRealSrc<T, StreamAB>{row0, h});
    eng.lds_to_lds(lds, twh);
  }
  cx<T>* dst = inter + static_cast<long long>(zl) * a.interZStride + y0;
  // post pass over the pairs (k, h - k): see x_forward_r2c_kernel
  for (int idx = threadIdx.x; idx < B * (h / 2 + 1); idx += blockDim.x) {
    const int b = idx % B, k = idx / B, m = h - k;
    if (b >= yl) continue;
    const int ck = xcol_of(a, xCol, k), cm = xcol_of(a, xCol, m);
    if (ck < 0 && cm < 0) continue;
    const cx<T> A = lds[eng.out_at(b, k == h ? 0 : k)];
    const cx<T> Bv = lds[eng.out_at(b, m == h ? 0 : m)];
    const cx<T> wk = twn[k];
    if (ck >= 0) {
      const cx<T> ym = conj(Bv);
      const cx<T> e = scale(A + ym, T(0.5));
      const cx<T> o = scale(rot<-1>(A - ym), T(0.5));
      st_inter(&dst[inter_row(a, ck) + b], e + twm<-1>(o, wk));
    }
    if (cm >= 0 && m != k) {
      const cx<T> ym = conj(A);
      const cx<T> e = scale(Bv + ym, T(0.5));
      const cx<T> o = scale(rot<-1>(Bv - ym), T(0.5));
      st_inter(&dst[inter_row(a, cm) + b], e + twm<-1>(o, mk<T>(-wk.x, wk.y)));
    }
  }
}

template <class Eng, typename T, bool StreamAB>
__global__ void __launch_bounds__(Eng::kBlock)
    x_forward_pair_r2c_kernel(Eng eng, XArgs a, const T* __restrict__ pa, const T* __restrict__ pb,
                              cx<T>* __restrict__ inter, const cx<T>* __restrict__ twh,
                              const cx<T>* __restrict__ twn) {
  x_forward_pair_r2c_body<Eng, T, StreamAB>(eng, a, pa, pb, inter, twh, twn);
}

// Batched launch: blockIdx.z selects the member, whose a is XArgs::batch.in,
// whose b is second.b (real arrays behind the cx<T> pointers of PairSecond) and
// whose intermediate is XArgs::batch.out.
template <class Eng, typename T, bool StreamAB>
__global__ void __launch_bounds__(Eng::kBlock)
    x_forward_pair_r2c_batch_kernel(Eng eng, XArgs a, PairSecond<T> second, const cx<T>* __restrict__ twh,
                                    const cx<T>* __restrict__ twn) {
  x_forward_pair_r2c_body<Eng, T, StreamAB>(eng, a, static_cast<const T*>(a.batch.in[blockIdx.z]),
                                            reinterpret_cast<const T*>(second.b[blockIdx.z]),
                                            static_cast<cx<T>*>(a.batch.out[blockIdx.z]), twh, twn);
}

// acc pair idx += w * {a.x lds[src(idx)].x, a.y lds[src(idx)].y} for idx in
// [0, total): fock_rows on packed-real rows (y.x = u[2m], y.y = u[2m+1]), a and
// acc read and written as pairs, kFockUnroll loads of each in flight. `pa` and
// `acc` must be aligned to one pair.
template <bool Stream, typename T, class Src>
__device__ __forceinline__ void fock_row_pairs(const cx<T>* lds, const cx<T>* __restrict__ pa,
                                               cx<T>* __restrict__ acc, T w, int total, Src src) {
  for (int base = threadIdx.x; base < total; base += blockDim.x * kFockUnroll) {
    cx<T> av[kFockUnroll], r[kFockUnroll];
#pragma unroll
    for (int u = 0; u < kFockUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        if constexpr (Stream) {
          av[u] = ld_stream(pa + idx);
          r[u] = ld_stream(acc + idx);
        } else {
          av[u] = pa[idx];
          r[u] = acc[idx];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kFockUnroll; ++u) {
      const int idx = base + u * static_cast<int>(blockDim.x);
      if (idx < total) {
        const cx<T> y = lds[src(idx)];
        const cx<T> o = mk<T>(fma(w * av[u].x, y.x, r[u].x), fma(w * av[u].y, y.y, r[u].y));
        if constexpr (Stream) st_stream(acc + idx, o);
        else acc[idx] = o;
      }
    }
  }
}

// Backward x stage of the pair operator (R2C, packed-real): step (a) of
// x_apply_r2c_kernel (c2r_rows_to_lds), then acc[2m] += w a[2m] y.x, acc[2m+1]
// += w a[2m+1] y.y on the workgroup's rows of acc straight from LDS. Tile, LDS
// layout (lines | Nyquist slot per line | xCol) and grid of the C2R launch. A
// workgroup owns its rows of acc: no atomics. StreamAcc: cache policy of a and acc.
template <class Eng, typename T, bool StreamAcc>
__global__ void __launch_bounds__(Eng::kBlock)
    x_backward_fock_r2c_kernel(Eng eng, XArgs a, const cx<T>* __restrict__ inter, const T* __restrict__ pa,
                               T* __restrict__ acc, T w, const cx<T>* __restrict__ twh,
                               const cx<T>* __restrict__ twn) {
  static_assert(!Eng::kBatchedCopy, "x backward fock r2c: compile-time engines only");
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int h = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<cx<T>*>(reinterpret_cast<char*>(lds) + eng.lds_bytes()) + B);
  build_xcol(a, xCol, h + 1);
  const int yl = min(B, a.Y - y0);
  c2r_rows_to_lds(eng, lds, a, xCol, inter + static_cast<long long>(zl) * a.interZStride + y0, yl, twh, twn);
  const long long off = (static_cast<long long>(zl) * a.Y + y0) * h;  // in pairs
  fock_row_pairs<StreamAcc>(lds, reinterpret_cast<const cx<T>*>(pa) + off, reinterpret_cast<cx<T>*>(acc) + off, w,
                            yl * h, [&](int idx) {
    const int b = idx / h;
    return eng.out_at(b, idx - b * h);
  });
}

// The pairs of a batched launch share acc: the workgroup that owns a tile loops
// over the members in list order (intermediates from XArgs::batch.in, a and
// weight from `members`, whose cx<T> pointers hold real arrays), as
// x_backward_fock_batch_kernel does. The sum order is fixed by the lane's own
// program order, without atomics; a and acc take the default cache policy
// because the members revisit the tile.
template <class Eng, typename T>
__global__ void __launch_bounds__(Eng::kBlock)
    x_backward_fock_r2c_batch_kernel(Eng eng, XArgs a, FockMembers<T> members, T* __restrict__ acc,
                                     const cx<T>* __restrict__ twh, const cx<T>* __restrict__ twn) {
  static_assert(!Eng::kBatchedCopy, "x backward fock r2c: compile-time engines only");
  SPFFT_LDS_DECL(T);
  const int B = eng.lines();
  const int h = eng.n();
  int tx, ty;
  block_tile(tx, ty);
  const int zl = a.zBegin + ty;
  const int y0 = tx * B;
  int* xCol = reinterpret_cast<int*>(reinterpret_cast<cx<T>*>(reinterpret_cast<char*>(lds) + eng.lds_bytes()) + B);
  build_xcol(a, xCol, h + 1);
  const int yl = min(B, a.Y - y0);
  const long long off = (static_cast<long long>(zl) * a.Y + y0) * h;  // in pairs
  for (int m = 0; m < a.batch.count; ++m) {
    // the twiddle tables are pinned anew for every member (see x_density_r2c_kernel)
    const cx<T>* twhM = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(twh)));
    const cx<T>* twnM = reinterpret_cast<const cx<T>*>(pin_uniform64(reinterpret_cast<long long>(twn)));
    if (m > 0) __syncthreads();  // the previous member's rows have been read
    c2r_rows_to_lds(eng, lds, a, xCol,
                    static_cast<const cx<T>*>(a.batch.in[m]) + static_cast<long long>(zl) * a.interZStride + y0, yl,
                    twhM, twnM);
    fock_row_pairs<false>(lds, members.a[m] + off, reinterpret_cast<cx<T>*>(acc) + off, members.w[m], yl * h,
                          [&](int idx) {
      const int b = idx / h;
      return eng.out_at(b, idx - b * h);
    });
  }
}

// Engines whose batched accumulating packed-real x stage keeps the member loop
// inside the workgroup (FockBandLoop of the C2C stage); the others run one
// single-pair launch per member, in order on the stream. The fp32 h = 512 and
// h = 1024 shapes do not keep it, as for the density (R2cDensityBandLoop): with
// the loop their kernels took all 256 VGPRs and 84 B and 284 B of scratch per
// lane (20 and 70 spilled registers).
template <class Eng>
struct R2cFockBandLoop {
  static constexpr bool value = true;
};
template <int S, bool LF, bool TwPre>
struct R2cFockBandLoop<CtEng<float, 512, S, LF, TwPre>> {
  static constexpr bool value = false;
};
template <int S, bool LF, bool TwPre>
struct R2cFockBandLoop<CtEng<float, 1024, S, LF, TwPre>> {
  static constexpr bool value = false;
};

// ------------------------------------------------------------ host helpers
RtPlan make_rt_plan(int n, std::size_t elemBytes);

// Bluestein plan and device tables of length n (cached per device), or
// nullptr-tables when n does not use Bluestein.
struct BlueTables {
  RtPlan pm;
  const void* chirp = nullptr;
  const void* filt = nullptr;
  const void* twm = nullptr;
};
bool use_bluestein(int n, std::size_t elemBytes);
// LDS bytes and lines per workgroup of the one-workgroup engine (run-time or
// Bluestein) of a length without a compile-time kernel; throws GPUFFTError when
// a line does not fit
std::size_t in_lds_engine_bytes(int n, std::size_t elemBytes, int& lines);
BlueTables bluestein_tables(int n, bool dbl);

template <class K>
inline void prepare_kernel(K kernel, std::size_t ldsBytes) {
  if (ldsBytes > 64 * 1024) {
    gpu_check(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(ldsBytes)),
              "hipFuncSetAttribute");
  }
}

// Calls f(engine, threads, lines, ldsBytes) with the CT engine of length n if
// there is one, else with the RT engine.
template <typename T, int S, bool LF = false, bool TwPre = true, class F>
inline void with_engine(int n, F&& f) {
  switch (n) {
#define SPFFT_CT_CASE(NN)                                                         \
  case NN: {                                                                      \
    using E = CtEng<T, NN, S, LF, TwPre>;                                                \
    f(E{}, E::h_threads(), E::h_lines(), E::h_lds());                             \
    return;                                                                       \
  }
    SPFFT_CT_CASE(16)
    SPFFT_CT_CASE(32)
    SPFFT_CT_CASE(64)
    SPFFT_CT_CASE(128)
    SPFFT_CT_CASE(256)
    SPFFT_CT_CASE(512)
    SPFFT_CT_CASE(1024)
#define SPFFT_MR_CASE(NN) SPFFT_CT_CASE(NN)
    SPFFT_MR_SIZES(SPFFT_MR_CASE)
#undef SPFFT_MR_CASE
#undef SPFFT_CT_CASE
    default: {
      if (use_bluestein(n, sizeof(cx<T>))) {
        const BlueTables bt = bluestein_tables(n, sizeof(T) == 8);
        BlueEng<T, S> e{bt.pm, n, static_cast<const cx<T>*>(bt.chirp),
                        static_cast<const cx<T>*>(bt.filt), static_cast<const cx<T>*>(bt.twm)};
        f(e, kMaxThreads, e.pm.lines, std::size_t(2) * e.pm.lines * e.pm.ls * sizeof(cx<T>));
        return;
      }
      RtEng<T, S, LF> e{make_rt_plan(n, sizeof(cx<T>))};
      f(e, kRtThreads, e.p.lines,
        std::size_t(e.p.inplace ? 1 : 2) * e.p.lines * e.p.ls * sizeof(cx<T>));
      return;
    }
  }
}

inline unsigned ceil_div(long long a, long long b) { return static_cast<unsigned>((a + b - 1) / b); }

}  // namespace dev
}  // namespace spfft
