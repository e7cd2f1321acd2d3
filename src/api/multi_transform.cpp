// Overlapped execution of independent transforms
// (reference: src/spfft/multi_transform_internal.hpp:47-145).
//
// GPU transforms each own a stream, so enqueuing stage k of every transform
// before stage k+1 lets the GPU overlap transform i's exchange with transform
// j's FFT kernels; host transforms run their stages in between.
#include <algorithm>
#include <set>
#include <vector>

#include "api/transform_impl.hpp"
#include "core/timing.hpp"
#include "spfft/multi_transform.hpp"
#include "spfft/multi_transform_float.hpp"

namespace spfft {
namespace {

template <typename T>
void check_distinct_grids(const std::vector<TransformImpl<T>*>& ts) {
  std::set<const GridImpl<T>*> grids;
  for (auto* t : ts) {
    if (!t) throw InvalidParameterError();
    if (!grids.insert(t->grid().get()).second) throw InvalidParameterError();
  }
}

// Batched groups (GpuExecutor::backward_batch / forward_batch): GPU transforms
// that can share launches, grouped by plan key in call order, at most
// dev::kMaxBatch per group; small grids batch join-free members only, large
// grids run sub-batches of batch_split() on their leaders' streams. Returns,
// per transform, whether a batch ran it. `tag(i)` must match within a group
// (the forward scaling).
template <typename T, class Eligible, class Tag, class Run>
std::vector<bool> run_batches(const std::vector<TransformImpl<T>*>& ts, Eligible eligible, Tag tag,
                              Run run) {
  const int n = static_cast<int>(ts.size());
  std::vector<bool> done(n, false);
  for (auto* t : ts)
    if (t->is_gpu()) t->gpu()->ensure_stream();  // the stream comparisons below need them
  auto ok = [&](int j) {
    return !done[j] && ts[j]->is_gpu() && ts[j]->gpu()->batchable() && eligible(j);
  };
  for (int i = 0; i < n; ++i) {
    if (!ok(i)) continue;
    GpuExecutor<T>* lead = ts[i]->gpu();
    const bool large = lead->batch_large();
    std::vector<int> group{i};
    for (int j = i + 1; j < n && static_cast<int>(group.size()) < dev::kMaxBatch; ++j)
      if (ok(j) && ts[j]->gpu()->batch_key() == lead->batch_key() && tag(j) == tag(i) &&
          (large || ts[j]->gpu()->batch_join_free(*lead)))
        group.push_back(j);
    if (group.size() < 2) continue;
    // sub-batches overlap only on different streams: one shared stream keeps one batch
    bool oneStream = true;
    for (int j : group) oneStream = oneStream && ts[j]->gpu()->stream() == lead->stream();
    const std::size_t split =
        large && !oneStream ? static_cast<std::size_t>(lead->batch_split()) : group.size();
    for (std::size_t k = 0; k < group.size(); k += split)
      run(std::vector<int>(group.begin() + k, group.begin() + std::min(group.size(), k + split)));
    for (int j : group) done[j] = true;
  }
  return done;
}

template <typename T>
void multi_forward(const std::vector<TransformImpl<T>*>& ts,
                   const SpfftProcessingUnitType* inputLocations, T* const* outputs,
                   const SpfftScalingType* scalings) {
  SPFFT_TIMED_SCOPE("multi_forward");
  check_distinct_grids(ts);
  const int n = static_cast<int>(ts.size());
  for (int i = 0; i < n; ++i)
    if (scalings[i] != SPFFT_NO_SCALING && scalings[i] != SPFFT_FULL_SCALING)
      throw InvalidParameterError();
  const std::vector<bool> batched = run_batches<T>(
      ts,
      [&](int i) {
        return inputLocations[i] == SPFFT_PU_GPU &&
               (ts[i]->plan().numLocalElements == 0 || is_device_pointer(outputs[i]));
      },
      [&](int i) { return static_cast<int>(scalings[i]); },
      [&](const std::vector<int>& g) {
        std::vector<GpuExecutor<T>*> ex;
        std::vector<T*> outs;
        for (int j : g) {
          ex.push_back(ts[j]->gpu());
          outs.push_back(outputs[j]);
        }
        GpuExecutor<T>::forward_batch(ex, outs, scalings[g[0]]);
      });
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) ts[i]->forward_xy(inputLocations[i]);
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      ts[i]->forward_xy(inputLocations[i]);
      ts[i]->forward_exchange(true);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) {
      ts[i]->forward_exchange(true);
      ts[i]->forward_z(outputs[i], scalings[i]);
    }
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) ts[i]->forward_z(outputs[i], scalings[i]);
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && ts[i]->gpu()->synchronous()) ts[i]->synchronize();
}

template <typename T>
void multi_backward(const std::vector<TransformImpl<T>*>& ts, const T* const* inputs,
                    const SpfftProcessingUnitType* outputLocations) {
  SPFFT_TIMED_SCOPE("multi_backward");
  check_distinct_grids(ts);
  const int n = static_cast<int>(ts.size());
  const std::vector<bool> batched = run_batches<T>(
      ts,
      [&](int i) {
        return outputLocations[i] == SPFFT_PU_GPU &&
               (ts[i]->plan().numLocalElements == 0 || is_device_pointer(inputs[i]));
      },
      [](int) { return 0; },
      [&](const std::vector<int>& g) {
        std::vector<GpuExecutor<T>*> ex;
        std::vector<const T*> ins;
        for (int j : g) {
          ex.push_back(ts[j]->gpu());
          ins.push_back(inputs[j]);
        }
        GpuExecutor<T>::backward_batch(ex, ins);
      });
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) ts[i]->backward_z(inputs[i]);
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      ts[i]->backward_z(inputs[i]);
      ts[i]->backward_exchange(true);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) {
      ts[i]->backward_exchange(true);
      ts[i]->backward_xy(outputLocations[i]);
    }
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) ts[i]->backward_xy(outputLocations[i]);
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && ts[i]->gpu()->synchronous()) ts[i]->synchronize();
}

// apply_local of every transform, phases interleaved like the directions above:
// fused GPU plans with equal keys share one launch per stage.
template <typename T>
void multi_apply_local(const std::vector<TransformImpl<T>*>& ts, const T* const* inputs,
                       const T* const* potentials, T* const* outputs,
                       const SpfftScalingType* scalings) {
  SPFFT_TIMED_SCOPE("multi_apply_local");
  check_distinct_grids(ts);
  const int n = static_cast<int>(ts.size());
  if (n > 0 && (!inputs || !potentials || !outputs || !scalings)) throw InvalidParameterError();
  for (int i = 0; i < n; ++i) {
    if (scalings[i] != SPFFT_NO_SCALING && scalings[i] != SPFFT_FULL_SCALING)
      throw InvalidParameterError();
    if (!potentials[i]) throw InvalidParameterError();
  }
  const std::vector<bool> batched = run_batches<T>(
      ts,
      [&](int i) {
        return ts[i]->apply_local_fused() && is_device_pointer(potentials[i]) &&
               ts[i]->gpu()->pairs_aligned(potentials[i]) &&
               (ts[i]->plan().numLocalElements == 0 ||
                (is_device_pointer(inputs[i]) && is_device_pointer(outputs[i])));
      },
      [&](int i) { return static_cast<int>(scalings[i]); },
      [&](const std::vector<int>& g) {
        std::vector<GpuExecutor<T>*> ex;
        std::vector<const T*> ins, pots;
        std::vector<T*> outs;
        for (int j : g) {
          ex.push_back(ts[j]->gpu());
          ins.push_back(inputs[j]);
          pots.push_back(potentials[j]);
          outs.push_back(outputs[j]);
        }
        GpuExecutor<T>::apply_local_batch(ex, ins, pots, outs, scalings[g[0]]);
      });
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) ts[i]->backward_z(inputs[i]);
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      ts[i]->backward_z(inputs[i]);
      ts[i]->backward_exchange(true);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) {
      ts[i]->backward_exchange(true);
      ts[i]->apply_local_xy(potentials[i]);
    }
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      ts[i]->apply_local_xy(potentials[i]);
      ts[i]->forward_exchange(true);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) {
      ts[i]->forward_exchange(true);
      ts[i]->forward_z(outputs[i], scalings[i]);
    }
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) ts[i]->forward_z(outputs[i], scalings[i]);
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && ts[i]->gpu()->synchronous()) ts[i]->synchronize();
}

// density += sum_i weights[i] |backward_i(inputs[i])|^2 into one shared rho, phases
// interleaved like multi_apply_local. The transforms update the same array, so
// their density stages run one after another: batches first (in group order),
// then the other GPU transforms and the host transforms in list order; `last`
// is the GPU executor whose stream holds the latest update, and the next stage
// on another stream waits for it by an event. The order depends on the call
// alone, so the same call on the same data gives the same bits.
template <typename T>
void multi_accumulate_density(const std::vector<TransformImpl<T>*>& ts, const T* const* inputs,
                              const T* weights, T* density) {
  SPFFT_TIMED_SCOPE("multi_accumulate_density");
  check_distinct_grids(ts);
  const int n = static_cast<int>(ts.size());
  if (n > 0 && (!inputs || !weights)) throw InvalidParameterError();
  for (int i = 0; i < n; ++i)
    if (!density && ts[i]->plan().local_planes() > 0) throw InvalidParameterError();
  GpuExecutor<T>* last = nullptr;
  const bool deviceRho = density && is_device_pointer(density);
  const std::vector<bool> batched = run_batches<T>(
      ts,
      [&](int i) {
        return ts[i]->density_fused() && deviceRho && ts[i]->gpu()->pairs_aligned(density) &&
               (ts[i]->plan().numLocalElements == 0 || is_device_pointer(inputs[i]));
      },
      [](int) { return 0; },
      [&](const std::vector<int>& g) {
        std::vector<GpuExecutor<T>*> ex;
        std::vector<const T*> ins;
        std::vector<T> ws;
        for (int j : g) {
          ex.push_back(ts[j]->gpu());
          ins.push_back(inputs[j]);
          ws.push_back(weights[j]);
        }
        GpuExecutor<T>::accumulate_density_batch(ex, ins, ws, density, last);
        last = ex[0];
      });
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) ts[i]->backward_z(inputs[i]);
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      ts[i]->backward_z(inputs[i]);
      ts[i]->backward_exchange(true);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) {
      ts[i]->backward_exchange(true);
      ts[i]->gpu()->accumulate_density_xy(density, weights[i], last);
      last = ts[i]->gpu();
    }
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      // a host transform updates rho on the calling thread: behind the GPU transforms' updates
      if (last) last->synchronize();
      last = nullptr;
      ts[i]->accumulate_density_xy(density, weights[i]);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && ts[i]->gpu()->synchronous()) ts[i]->synchronize();
}

// acc += sum_i weights[i] a[i] backward_i(K_i (scale forward_i(conj(a[i]) b[i]))) into
// one shared acc: the pairs of one band of the exchange operator. Plans with
// fused x and z stages and equal keys run as batches first (in group order),
// everything else per transform with the phases interleaved, in list order.
// Every update of acc is ordered behind the previous one as in
// multi_accumulate_density (`last`), so the sum order depends on the call alone.
// A host acc is staged by each GPU member in its own buffer: such members run
// strictly one after another, each behind a synchronize of the previous one, so
// that no staged copy is written back over a later update.
template <typename T>
void multi_accumulate_fock(const std::vector<TransformImpl<T>*>& ts, const T* const* a, const T* const* b,
                           const T* const* kernels, bool complexKernel, const T* weights, T* acc,
                           SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("multi_accumulate_fock");
  check_distinct_grids(ts);
  const int n = static_cast<int>(ts.size());
  if (n > 0 && (!a || !b || !kernels || !weights)) throw InvalidParameterError();
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  for (int i = 0; i < n; ++i) {
    const IndexPlan& p = ts[i]->plan();
    const IndexPlan& p0 = ts[0]->plan();
    // one acc: one local space domain, complex or real
    if (p.type != p0.type || p.dimX != p0.dimX || p.dimY != p0.dimY || p.local_planes() != p0.local_planes())
      throw InvalidParameterError();
    if (p.local_planes() > 0 && (!acc || !a[i] || !b[i])) throw InvalidParameterError();
    if (p.numLocalElements > 0 && !kernels[i]) throw InvalidParameterError();
  }
  GpuExecutor<T>* last = nullptr;
  const bool deviceAcc = acc && is_device_pointer(acc);
  const std::vector<bool> batched = run_batches<T>(
      ts,
      [&](int i) {
        const IndexPlan& p = ts[i]->plan();
        // (a packed-real R2C pair plan reads a, b and acc as pairs: members with a
        // misaligned array take the per-transform path, which runs them composed)
        const bool pairs = ts[i]->fock_r2c_fused() && ts[i]->gpu()->fock_pairs_aligned(a[i]) &&
                           ts[i]->gpu()->fock_pairs_aligned(b[i]) && ts[i]->gpu()->fock_pairs_aligned(acc);
        return (ts[i]->fock_fused() || pairs) && ts[i]->reciprocal_fused() && deviceAcc &&
               (p.local_planes() == 0 || (is_device_pointer(a[i]) && is_device_pointer(b[i]))) &&
               (p.numLocalElements == 0 || is_device_pointer(kernels[i]));
      },
      [](int) { return 0; },
      [&](const std::vector<int>& g) {
        std::vector<GpuExecutor<T>*> ex;
        std::vector<const T*> as, bs, ks;
        std::vector<T> ws;
        for (int j : g) {
          ex.push_back(ts[j]->gpu());
          as.push_back(a[j]);
          bs.push_back(b[j]);
          ks.push_back(kernels[j]);
          ws.push_back(weights[j]);
        }
        GpuExecutor<T>::accumulate_fock_batch(ex, as, bs, ks, complexKernel, ws, acc, scaling, last);
        last = ex[0];
      });
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) ts[i]->fock_forward_xy(a[i], b[i]);
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      ts[i]->fock_forward_xy(a[i], b[i]);
      ts[i]->forward_exchange(true);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) {
      ts[i]->forward_exchange(true);
      ts[i]->reciprocal_z(kernels[i], complexKernel, nullptr, scaling);
    }
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      ts[i]->reciprocal_z(kernels[i], complexKernel, nullptr, scaling);
      ts[i]->backward_exchange(true);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && !batched[i]) {
      ts[i]->backward_exchange(true);
      if (!deviceAcc && last) {
        last->synchronize();  // its copy of acc is back on the host
        last = nullptr;
      }
      ts[i]->gpu()->fock_backward_xy(a[i], acc, weights[i], last);
      last = ts[i]->gpu();
    }
  for (int i = 0; i < n; ++i)
    if (!ts[i]->is_gpu()) {
      // a host transform updates acc on the calling thread: behind the GPU transforms' updates
      if (last) last->synchronize();
      last = nullptr;
      ts[i]->fock_backward_xy(a[i], acc, weights[i]);
    }
  for (int i = 0; i < n; ++i)
    if (ts[i]->is_gpu() && ts[i]->gpu()->synchronous()) ts[i]->synchronize();
}

// ---------------------------------------------- reciprocal fan-out and fan-in
// out = in * K or out += in * K over `count` interleaved complex host values
// (the multiply of TransformImpl::reciprocal_z)
template <typename T>
void host_values_scale(T* out, const T* in, const T* kernel, bool complexKernel, std::size_t count, bool add) {
  for (std::size_t i = 0; i < count; ++i) {
    const T re = in[2 * i], im = in[2 * i + 1];
    T pr, pi;
    if (complexKernel) {
      pr = re * kernel[2 * i] - im * kernel[2 * i + 1];
      pi = re * kernel[2 * i + 1] + im * kernel[2 * i];
    } else {
      pr = re * kernel[i];
      pi = im * kernel[i];
    }
    out[2 * i] = add ? out[2 * i] + pr : pr;
    out[2 * i + 1] = add ? out[2 * i + 1] + pi : pi;
  }
}

// The checks both fan operators share; returns whether the fused z stage runs:
// GPU transforms with device space domains, reciprocal_fan_fused plans with
// equal keys, at most dev::kMaxBatch of them, device kernels.
template <typename T>
bool check_fan(const std::vector<TransformImpl<T>*>& ts, SpfftProcessingUnitType location,
               const T* const* kernels, SpfftScalingType scaling) {
  check_distinct_grids(ts);
  const int n = static_cast<int>(ts.size());
  if (n > 0 && !kernels) throw InvalidParameterError();
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  if (location != SPFFT_PU_HOST && location != SPFFT_PU_GPU) throw InvalidParameterError();
  for (int i = 0; i < n; ++i) {
    const IndexPlan& p = ts[i]->plan();
    const IndexPlan& p0 = ts[0]->plan();
    // values are matched by position, space domains by element
    if (p.type != p0.type || p.dimX != p0.dimX || p.dimY != p0.dimY || p.dimZ != p0.dimZ ||
        p.local_planes() != p0.local_planes() || p.numLocalElements != p0.numLocalElements)
      throw InvalidParameterError();
    if (!ts[i]->is_gpu() && location != SPFFT_PU_HOST) throw InvalidParameterError();
    if (p.numLocalElements > 0 && !kernels[i]) throw InvalidParameterError();
  }
  if (n < 2 || n > dev::kMaxBatch || location != SPFFT_PU_GPU) return false;
  for (int i = 0; i < n; ++i) {
    if (!ts[i]->is_gpu()) return false;
    ts[i]->gpu()->ensure_stream();
    if (!ts[i]->gpu()->reciprocal_fan_fused() || ts[i]->gpu()->batch_key() != ts[0]->gpu()->batch_key())
      return false;
    if (ts[i]->plan().numLocalElements > 0 && !is_device_pointer(kernels[i])) return false;
  }
  return true;
}

// space_i = backward_i(K_i * c) for every member, c = scale * forward_0(space_0);
// `values` (may be NULL) receives c. Fused plans run GpuExecutor::
// reciprocal_fan_out_batch; everything else the composition per transform in
// list order: forward_0 into a values buffer, then per member the multiply of
// the values and backward_i (device buffers when every transform is a GPU
// transform, host buffers otherwise).
template <typename T>
void multi_reciprocal_fan_out(const std::vector<TransformImpl<T>*>& ts, SpfftProcessingUnitType location,
                              const T* const* kernels, bool complexKernel, T* values,
                              SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("multi_reciprocal_fan_out");
  bool fused = check_fan<T>(ts, location, kernels, scaling);
  const int n = static_cast<int>(ts.size());
  if (n == 0) return;
  if (n == 1) {
    ts[0]->apply_reciprocal(location, kernels[0], complexKernel, values, scaling);
    return;
  }
  const std::size_t count = static_cast<std::size_t>(ts[0]->plan().numLocalElements);
  if (values && count > 0 && !is_device_pointer(values)) fused = false;
  if (fused) {
    std::vector<GpuExecutor<T>*> ex;
    std::vector<const T*> ks;
    for (int i = 0; i < n; ++i) {
      ex.push_back(ts[i]->gpu());
      ks.push_back(kernels[i]);
    }
    GpuExecutor<T>::reciprocal_fan_out_batch(ex, ks, complexKernel, values, scaling);
    for (int i = 0; i < n; ++i)
      if (ts[i]->gpu()->synchronous()) ts[i]->synchronize();
    return;
  }
  bool allGpu = true;
  for (auto* t : ts) allGpu = allGpu && t->is_gpu();
  if (allGpu) {
    GpuExecutor<T>* g0 = ts[0]->gpu();
    const bool hostValues = values && count > 0 && !is_device_pointer(values);
    cx<T>* c = values && !hostValues ? reinterpret_cast<cx<T>*>(values) : g0->fan_buffer(0);
    ts[0]->forward_xy(location);
    ts[0]->forward_exchange(false);
    ts[0]->forward_z(reinterpret_cast<T*>(c), scaling);
    if (hostValues) g0->download_values(values, c);
    ts[0]->synchronize();  // c is complete: the members' streams may read it
    for (int i = 0; i < n; ++i) {
      GpuExecutor<T>* g = ts[i]->gpu();
      cx<T>* prod = g->fan_buffer(1);
      g->values_scale(prod, c, kernels[i], complexKernel, false);
      ts[i]->backward_z(reinterpret_cast<const T*>(prod));
      ts[i]->backward_exchange(false);
      ts[i]->backward_xy(location);
    }
    // (also in asynchronous mode: c may be member 0's work array, which its next call reuses)
    for (int i = 0; i < n; ++i) ts[i]->synchronize();
    return;
  }
  std::vector<T> c(2 * std::max<std::size_t>(count, 1)), prod(c.size());
  ts[0]->forward(location, c.data(), scaling);
  ts[0]->synchronize();
  if (values) {
    if (count > 0 && is_device_pointer(values)) throw InvalidParameterError();
    std::copy(c.begin(), c.begin() + 2 * count, values);
  }
  for (int i = 0; i < n; ++i) {
    host_values_scale<T>(prod.data(), c.data(), kernels[i], complexKernel, count, false);
    ts[i]->backward(prod.data(), location);
    ts[i]->synchronize();
  }
}

// space_0 = backward_0(sum_i K_i * (scale * forward_i(space_i))), summed in list
// order; the other members' space domains are only read. Fused plans run
// GpuExecutor::reciprocal_fan_in_batch; everything else the composition per
// transform in list order: forward_i and a multiply-add into one values buffer,
// each update behind the previous one, then backward_0.
template <typename T>
void multi_reciprocal_fan_in(const std::vector<TransformImpl<T>*>& ts, SpfftProcessingUnitType location,
                             const T* const* kernels, bool complexKernel, SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("multi_reciprocal_fan_in");
  const bool fused = check_fan<T>(ts, location, kernels, scaling);
  const int n = static_cast<int>(ts.size());
  if (n == 0) return;
  if (n == 1) {
    ts[0]->apply_reciprocal(location, kernels[0], complexKernel, nullptr, scaling);
    return;
  }
  const std::size_t count = static_cast<std::size_t>(ts[0]->plan().numLocalElements);
  if (fused) {
    std::vector<GpuExecutor<T>*> ex;
    std::vector<const T*> ks;
    for (int i = 0; i < n; ++i) {
      ex.push_back(ts[i]->gpu());
      ks.push_back(kernels[i]);
    }
    GpuExecutor<T>::reciprocal_fan_in_batch(ex, ks, complexKernel, scaling);
    for (int i = 0; i < n; ++i)
      if (ts[i]->gpu()->synchronous()) ts[i]->synchronize();
    return;
  }
  bool allGpu = true;
  for (auto* t : ts) allGpu = allGpu && t->is_gpu();
  if (allGpu) {
    cx<T>* sum = ts[0]->gpu()->fan_buffer(0);
    for (int i = 0; i < n; ++i) {
      GpuExecutor<T>* g = ts[i]->gpu();
      cx<T>* c = g->fan_buffer(1);
      ts[i]->forward_xy(location);
      ts[i]->forward_exchange(false);
      ts[i]->forward_z(reinterpret_cast<T*>(c), scaling);
      g->values_scale(sum, c, kernels[i], complexKernel, i > 0);
      ts[i]->synchronize();  // the next member's update of the sum comes behind this one
    }
    ts[0]->backward_z(reinterpret_cast<const T*>(sum));
    ts[0]->backward_exchange(false);
    ts[0]->backward_xy(location);
    if (ts[0]->gpu()->synchronous()) ts[0]->synchronize();
    return;
  }
  std::vector<T> c(2 * std::max<std::size_t>(count, 1)), sum(c.size());
  for (int i = 0; i < n; ++i) {
    ts[i]->forward(location, c.data(), scaling);
    ts[i]->synchronize();
    host_values_scale<T>(sum.data(), c.data(), kernels[i], complexKernel, count, i > 0);
  }
  ts[0]->backward(sum.data(), location);
  ts[0]->synchronize();
}

// ------------------------------------------------------------------ value fans
// The checks both value fans share; returns whether the fused z fan stages
// run: GPU transforms with values_fan_fused plans and equal keys, at most
// dev::kMaxBatch of them, device kernels. `input` and the other arrays are
// checked by the callers.
template <typename T>
bool check_values_fan(const std::vector<TransformImpl<T>*>& ts, const T* const* kernelsA,
                      const T* const* kernelsB, bool twoLists) {
  check_distinct_grids(ts);
  const int n = static_cast<int>(ts.size());
  if (n > 0 && (!kernelsA || (twoLists && !kernelsB))) throw InvalidParameterError();
  for (int i = 0; i < n; ++i) {
    const IndexPlan& p = ts[i]->plan();
    const IndexPlan& p0 = ts[0]->plan();
    // values are matched by position, space domains by element
    if (p.type != p0.type || p.dimX != p0.dimX || p.dimY != p0.dimY || p.dimZ != p0.dimZ ||
        p.local_planes() != p0.local_planes() || p.numLocalElements != p0.numLocalElements)
      throw InvalidParameterError();
  }
  if (n < 1 || n > dev::kMaxBatch) return false;
  for (int i = 0; i < n; ++i) {
    if (!ts[i]->is_gpu()) return false;
    ts[i]->gpu()->ensure_stream();
    if (!ts[i]->gpu()->values_fan_fused() || ts[i]->gpu()->batch_key() != ts[0]->gpu()->batch_key())
      return false;
    if (kernelsA[i] && !is_device_pointer(kernelsA[i])) return false;
    if (twoLists && kernelsB[i] && !is_device_pointer(kernelsB[i])) return false;
  }
  return true;
}

// prod = K * in over the local values on g's stream (K null: in itself); the
// array the member's backward z stage reads
template <typename T>
const T* fan_scaled_values(GpuExecutor<T>* g, const cx<T>* in, const T* kernel, bool complexKernel) {
  if (!kernel) return reinterpret_cast<const T*>(in);
  cx<T>* prod = g->fan_buffer(1);
  g->values_scale(prod, in, kernel, complexKernel, false);
  return reinterpret_cast<const T*>(prod);
}

// the values as a device array: `input` itself, or a copy in g's fan buffer 3
template <typename T>
const cx<T>* fan_device_input(GpuExecutor<T>* g, const T* input, std::size_t count) {
  if (count == 0 || is_device_pointer(input)) return reinterpret_cast<const cx<T>*>(input);
  cx<T>* in = g->fan_buffer(3);
  g->copy_values(reinterpret_cast<T*>(in), input);
  g->synchronize();  // the members' streams may read it
  return in;
}

// density += sum_i weights[i] |backward_i(K_i * input)|^2 in list order. Fused
// plans run GpuExecutor::accumulate_density_fan_batch; everything else the
// composition per member in list order: a multiply of the values into a work
// buffer (none for a null kernel), then accumulate_density, each update of rho
// behind the previous one (device buffers when every transform is a GPU
// transform, host buffers otherwise).
template <typename T>
void multi_accumulate_density_fan(const std::vector<TransformImpl<T>*>& ts, const T* input,
                                  const T* const* kernels, bool complexKernel, const T* weights,
                                  T* density) {
  SPFFT_TIMED_SCOPE("multi_accumulate_density_fan");
  bool fused = check_values_fan<T>(ts, kernels, nullptr, false);
  const int n = static_cast<int>(ts.size());
  if (n == 0) return;
  if (!weights) throw InvalidParameterError();
  const IndexPlan& p0 = ts[0]->plan();
  const std::size_t count = static_cast<std::size_t>(p0.numLocalElements);
  if ((count > 0 && !input) || (p0.local_planes() > 0 && !density)) throw InvalidParameterError();
  if ((count > 0 && !is_device_pointer(input)) || (p0.local_planes() > 0 && !is_device_pointer(density)))
    fused = false;
  if (fused) {
    std::vector<GpuExecutor<T>*> ex;
    std::vector<const T*> ks;
    std::vector<T> ws;
    for (int i = 0; i < n; ++i) {
      ex.push_back(ts[i]->gpu());
      ks.push_back(kernels[i]);
      ws.push_back(weights[i]);
    }
    GpuExecutor<T>::accumulate_density_fan_batch(ex, input, ks, complexKernel, ws, density);
    for (int i = 0; i < n; ++i)
      if (ts[i]->gpu()->synchronous()) ts[i]->synchronize();
    return;
  }
  bool allGpu = true;
  for (auto* t : ts) allGpu = allGpu && t->is_gpu();
  if (allGpu) {
    const cx<T>* in = fan_device_input<T>(ts[0]->gpu(), input, count);
    for (int i = 0; i < n; ++i) {
      ts[i]->accumulate_density(fan_scaled_values<T>(ts[i]->gpu(), in, kernels[i], complexKernel), weights[i],
                                density);
      ts[i]->synchronize();  // the next member's update of rho comes behind this one
    }
    return;
  }
  if (count > 0 && is_device_pointer(input)) throw InvalidParameterError();
  std::vector<T> prod(2 * std::max<std::size_t>(count, 1));
  for (int i = 0; i < n; ++i) {
    if (kernels[i] && count > 0 && is_device_pointer(kernels[i])) throw InvalidParameterError();
    const T* src = input;
    if (kernels[i]) {
      host_values_scale<T>(prod.data(), input, kernels[i], complexKernel, count, false);
      src = prod.data();
    }
    ts[i]->accumulate_density(src, weights[i], density);
    ts[i]->synchronize();
  }
}

// output = sum_i L_i * (scale * forward_i(V_i * backward_i(K_i * input))) in
// list order. Fused plans run GpuExecutor::apply_local_fan_batch; everything
// else the composition per member in list order: a multiply of the values into
// a work buffer, apply_local into a second one, a multiply-add into the sum
// (null kernels skip the multiplies); `output` is written at the end, so it
// may be `input`.
template <typename T>
void multi_apply_local_fan(const std::vector<TransformImpl<T>*>& ts, const T* input,
                           const T* const* kernelsIn, const T* const* potentials,
                           const T* const* kernelsOut, bool complexKernel, T* output,
                           SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("multi_apply_local_fan");
  bool fused = check_values_fan<T>(ts, kernelsIn, kernelsOut, true);
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  const int n = static_cast<int>(ts.size());
  if (n == 0) return;
  if (!potentials) throw InvalidParameterError();
  const IndexPlan& p0 = ts[0]->plan();
  const std::size_t count = static_cast<std::size_t>(p0.numLocalElements);
  if (count > 0 && (!input || !output)) throw InvalidParameterError();
  for (int i = 0; i < n; ++i) {
    if (p0.local_planes() > 0 && !potentials[i]) throw InvalidParameterError();
    if (p0.local_planes() > 0 && !is_device_pointer(potentials[i])) fused = false;
  }
  if (count > 0 && (!is_device_pointer(input) || !is_device_pointer(output))) fused = false;
  if (fused) {
    std::vector<GpuExecutor<T>*> ex;
    std::vector<const T*> kin, pots, kout;
    for (int i = 0; i < n; ++i) {
      ex.push_back(ts[i]->gpu());
      kin.push_back(kernelsIn[i]);
      pots.push_back(potentials[i]);
      kout.push_back(kernelsOut[i]);
    }
    GpuExecutor<T>::apply_local_fan_batch(ex, input, kin, pots, kout, complexKernel, output, scaling);
    for (int i = 0; i < n; ++i)
      if (ts[i]->gpu()->synchronous()) ts[i]->synchronize();
    return;
  }
  bool allGpu = true;
  for (auto* t : ts) allGpu = allGpu && t->is_gpu();
  if (allGpu) {
    GpuExecutor<T>* g0 = ts[0]->gpu();
    const cx<T>* in = fan_device_input<T>(g0, input, count);
    cx<T>* sum = g0->fan_buffer(0);
    for (int i = 0; i < n; ++i) {
      GpuExecutor<T>* g = ts[i]->gpu();
      // member 0 with the identity L writes the sum itself
      cx<T>* res = i == 0 && !kernelsOut[i] ? sum : g->fan_buffer(2);
      ts[i]->apply_local(fan_scaled_values<T>(g, in, kernelsIn[i], complexKernel), potentials[i],
                         reinterpret_cast<T*>(res), scaling);
      if (kernelsOut[i]) g->values_scale(sum, res, kernelsOut[i], complexKernel, i > 0);
      else if (i > 0) g->values_add(sum, res);
      ts[i]->synchronize();  // the next member's update of the sum comes behind this one
    }
    g0->copy_values(output, reinterpret_cast<const T*>(sum));
    // (also in asynchronous mode: the sum is member 0's work array, which its next call reuses)
    ts[0]->synchronize();
    return;
  }
  if (count > 0 && (is_device_pointer(input) || is_device_pointer(output))) throw InvalidParameterError();
  std::vector<T> prod(2 * std::max<std::size_t>(count, 1)), res(prod.size()), sum(prod.size());
  for (int i = 0; i < n; ++i) {
    if (count > 0 && ((kernelsIn[i] && is_device_pointer(kernelsIn[i])) ||
                      (kernelsOut[i] && is_device_pointer(kernelsOut[i]))))
      throw InvalidParameterError();
    const T* src = input;
    if (kernelsIn[i]) {
      host_values_scale<T>(prod.data(), input, kernelsIn[i], complexKernel, count, false);
      src = prod.data();
    }
    ts[i]->apply_local(src, potentials[i], res.data(), scaling);
    ts[i]->synchronize();
    if (kernelsOut[i]) {
      host_values_scale<T>(sum.data(), res.data(), kernelsOut[i], complexKernel, count, i > 0);
    } else {
      for (std::size_t k = 0; k < 2 * count; ++k) sum[k] = i > 0 ? sum[k] + res[k] : res[k];
    }
  }
  std::copy(sum.begin(), sum.begin() + 2 * count, output);
}

// ------------------------------------------------------------ spinor operators
// The checks both spinor calls share over the 2S members {up_0, dn_0, ...};
// returns whether the fused x stages run: GPU transforms with spinor_fused
// plans and equal keys. The arrays are checked by the callers.
template <typename T>
bool check_spinors(const std::vector<TransformImpl<T>*>& ts) {
  check_distinct_grids(ts);
  const int n = static_cast<int>(ts.size());
  for (int i = 0; i < n; ++i) {
    const IndexPlan& p = ts[i]->plan();
    const IndexPlan& p0 = ts[0]->plan();
    // a real space domain cannot hold the off-diagonal term
    if (p.type != SPFFT_TRANS_C2C) throw InvalidParameterError();
    // values are matched by position, space domains by element
    if (p.dimX != p0.dimX || p.dimY != p0.dimY || p.dimZ != p0.dimZ || p.local_planes() != p0.local_planes() ||
        p.numLocalElements != p0.numLocalElements)
      throw InvalidParameterError();
  }
  for (int i = 0; i < n; ++i) {
    if (!ts[i]->is_gpu()) return false;
    ts[i]->gpu()->ensure_stream();
    if (!ts[i]->gpu()->spinor_fused() || ts[i]->gpu()->batch_key() != ts[0]->gpu()->batch_key()) return false;
  }
  return n > 0;
}

// Both members' backward results in host memory (host transforms, or a host
// and a GPU member): the space domains the host loops below work on.
template <typename T>
void spinor_host_backward(TransformImpl<T>* up, TransformImpl<T>* dn, const T* inUp, const T* inDn, T*& su,
                          T*& sd) {
  up->backward(inUp, SPFFT_PU_HOST);
  dn->backward(inDn, SPFFT_PU_HOST);
  up->synchronize();
  dn->synchronize();
  su = up->space_domain_data(SPFFT_PU_HOST);
  sd = dn->space_domain_data(SPFFT_PU_HOST);
}

// out_up = scale forward_up(v_uu psi_up + v_ud psi_dn), out_dn = scale
// forward_dn(conj(v_ud) psi_up + v_dd psi_dn) per spinor, psi = backward(in).
// Fused plans with device arrays run GpuExecutor::apply_local_spinor_batch in
// groups of dev::kMaxSpinors spinors in list order; everything else the
// composition per spinor in list order: backward of both members into their
// space domains, the 2x2 mix of the two space domains (a kernel on the up
// member's stream, or a loop on the host), forward of both.
template <typename T>
void multi_apply_local_spinor(const std::vector<TransformImpl<T>*>& ts, const T* const* inputs,
                              const T* const* potential, T* const* outputs, SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("multi_apply_local_spinor");
  bool fused = check_spinors<T>(ts);
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  const int n = static_cast<int>(ts.size());
  if (n == 0) return;
  if (!inputs || !potential || !outputs) throw InvalidParameterError();
  const IndexPlan& p0 = ts[0]->plan();
  const std::size_t count = static_cast<std::size_t>(p0.numLocalElements);
  const std::size_t space = static_cast<std::size_t>(p0.local_planes()) * p0.dimY * p0.dimX;
  for (int k = 0; k < 4; ++k) {
    if (space > 0 && !potential[k]) throw InvalidParameterError();
    if (space > 0 && !is_device_pointer(potential[k])) fused = false;
  }
  for (int i = 0; i < n; ++i) {
    if (count > 0 && (!inputs[i] || !outputs[i])) throw InvalidParameterError();
    if (count > 0 && (!is_device_pointer(inputs[i]) || !is_device_pointer(outputs[i]))) fused = false;
  }
  if (fused) {
    for (int i = 0; i < n; i += 2 * dev::kMaxSpinors) {
      const int e = std::min(n, i + 2 * dev::kMaxSpinors);
      std::vector<GpuExecutor<T>*> ex;
      std::vector<const T*> ins;
      std::vector<T*> outs;
      for (int j = i; j < e; ++j) {
        ex.push_back(ts[j]->gpu());
        ins.push_back(inputs[j]);
        outs.push_back(outputs[j]);
      }
      GpuExecutor<T>::apply_local_spinor_batch(ex, ins, potential, outs, scaling);
    }
    for (int i = 0; i < n; ++i)
      if (ts[i]->gpu()->synchronous()) ts[i]->synchronize();
    return;
  }
  for (int i = 0; i < n; i += 2) {
    TransformImpl<T>* up = ts[i];
    TransformImpl<T>* dn = ts[i + 1];
    if (up->is_gpu() && dn->is_gpu()) {
      up->backward(inputs[i], SPFFT_PU_GPU);
      dn->backward(inputs[i + 1], SPFFT_PU_GPU);
      up->gpu()->spinor_mix_space(dn->gpu(), potential);
      up->forward(SPFFT_PU_GPU, outputs[i], scaling);
      dn->forward(SPFFT_PU_GPU, outputs[i + 1], scaling);
      // the staged potential and the space domains are free for the next spinor
      up->synchronize();
      dn->synchronize();
      continue;
    }
    for (int k = 0; k < 4; ++k)
      if (space > 0 && is_device_pointer(potential[k])) throw InvalidParameterError();
    T *su = nullptr, *sd = nullptr;
    spinor_host_backward<T>(up, dn, inputs[i], inputs[i + 1], su, sd);
    for (std::size_t r = 0; r < space; ++r) {
      const T vuu = potential[0][r], vdd = potential[1][r], vre = potential[2][r], vim = potential[3][r];
      const T ux = su[2 * r], uy = su[2 * r + 1], dx = sd[2 * r], dy = sd[2 * r + 1];
      su[2 * r] = vuu * ux + (vre * dx - vim * dy);
      su[2 * r + 1] = vuu * uy + (vre * dy + vim * dx);
      sd[2 * r] = vdd * dx + (vre * ux + vim * uy);
      sd[2 * r + 1] = vdd * dy + (vre * uy - vim * ux);
    }
    up->forward(SPFFT_PU_HOST, outputs[i], scaling);
    dn->forward(SPFFT_PU_HOST, outputs[i + 1], scaling);
    up->synchronize();
    dn->synchronize();
  }
}

// n_uu += sum_s w_s |psi_up|^2, n_dd += sum_s w_s |psi_dn|^2, n_ud += sum_s w_s
// psi_up conj(psi_dn), in list order. Fused plans with device arrays run
// GpuExecutor::accumulate_spin_density_batch in groups of dev::kMaxSpinors
// spinors, one group behind the other on the leaders' streams; everything else
// per spinor in list order: backward of both members, then one pass over the
// two space domains (a kernel on the up member's stream, or a loop on the
// host), each update behind the previous one.
template <typename T>
void multi_accumulate_spin_density(const std::vector<TransformImpl<T>*>& ts, const T* const* inputs,
                                   const T* weights, T* const* density) {
  SPFFT_TIMED_SCOPE("multi_accumulate_spin_density");
  bool fused = check_spinors<T>(ts);
  const int n = static_cast<int>(ts.size());
  if (n == 0) return;
  if (!inputs || !weights || !density) throw InvalidParameterError();
  const IndexPlan& p0 = ts[0]->plan();
  const std::size_t count = static_cast<std::size_t>(p0.numLocalElements);
  const std::size_t space = static_cast<std::size_t>(p0.local_planes()) * p0.dimY * p0.dimX;
  for (int k = 0; k < 4; ++k) {
    if (space > 0 && !density[k]) throw InvalidParameterError();
    for (int j = 0; j < k; ++j)
      if (space > 0 && density[k] == density[j]) throw InvalidParameterError();
    if (space > 0 && !is_device_pointer(density[k])) fused = false;
  }
  for (int i = 0; i < n; ++i) {
    if (count > 0 && !inputs[i]) throw InvalidParameterError();
    if (count > 0 && !is_device_pointer(inputs[i])) fused = false;
  }
  if (fused) {
    GpuExecutor<T>* prev = nullptr;
    for (int i = 0; i < n; i += 2 * dev::kMaxSpinors) {
      const int e = std::min(n, i + 2 * dev::kMaxSpinors);
      std::vector<GpuExecutor<T>*> ex;
      std::vector<const T*> ins;
      std::vector<T> ws;
      for (int j = i; j < e; ++j) {
        ex.push_back(ts[j]->gpu());
        ins.push_back(inputs[j]);
        if ((j - i) % 2 == 0) ws.push_back(weights[j / 2]);
      }
      // a group's update of the arrays comes behind the previous group's
      GpuExecutor<T>::accumulate_spin_density_batch(ex, ins, ws, density, prev);
      prev = ex[0];
    }
    for (int i = 0; i < n; ++i)
      if (ts[i]->gpu()->synchronous()) ts[i]->synchronize();
    return;
  }
  for (int i = 0; i < n; i += 2) {
    TransformImpl<T>* up = ts[i];
    TransformImpl<T>* dn = ts[i + 1];
    const T w = weights[i / 2];
    if (up->is_gpu() && dn->is_gpu()) {
      up->backward(inputs[i], SPFFT_PU_GPU);
      dn->backward(inputs[i + 1], SPFFT_PU_GPU);
      up->gpu()->spin_density_space(dn->gpu(), density, w);
      // the next spinor's update of the arrays comes behind this one
      up->synchronize();
      dn->synchronize();
      continue;
    }
    for (int k = 0; k < 4; ++k)
      if (space > 0 && is_device_pointer(density[k])) throw InvalidParameterError();
    T *su = nullptr, *sd = nullptr;
    spinor_host_backward<T>(up, dn, inputs[i], inputs[i + 1], su, sd);
    for (std::size_t r = 0; r < space; ++r) {
      const T ux = su[2 * r], uy = su[2 * r + 1], dx = sd[2 * r], dy = sd[2 * r + 1];
      density[0][r] += w * (ux * ux + uy * uy);
      density[1][r] += w * (dx * dx + dy * dy);
      density[2][r] += w * (ux * dx + uy * dy);
      density[3][r] += w * (uy * dx - ux * dy);
    }
  }
}

template <typename TR, typename T>
std::vector<TransformImpl<T>*> impls(int n, TR* transforms) {
  if (n < 0 || (n > 0 && !transforms)) throw InvalidParameterError();
  std::vector<TransformImpl<T>*> v;
  for (int i = 0; i < n; ++i) v.push_back(transforms[i].impl().get());
  return v;
}

}  // namespace

void multi_transform_forward(int numTransforms, Transform* transforms,
                             SpfftProcessingUnitType* inputLocations, double** outputPointers,
                             SpfftScalingType* scalingTypes) {
  multi_forward<double>(impls<Transform, double>(numTransforms, transforms), inputLocations,
                        outputPointers, scalingTypes);
}

void multi_transform_backward(int numTransforms, Transform* transforms, double** inputPointers,
                              SpfftProcessingUnitType* outputLocations) {
  multi_backward<double>(impls<Transform, double>(numTransforms, transforms), inputPointers,
                         outputLocations);
}

void multi_transform_forward(int numTransforms, TransformFloat* transforms,
                             SpfftProcessingUnitType* inputLocations, float** outputPointers,
                             SpfftScalingType* scalingTypes) {
  multi_forward<float>(impls<TransformFloat, float>(numTransforms, transforms), inputLocations,
                       outputPointers, scalingTypes);
}

void multi_transform_backward(int numTransforms, TransformFloat* transforms, float** inputPointers,
                              SpfftProcessingUnitType* outputLocations) {
  multi_backward<float>(impls<TransformFloat, float>(numTransforms, transforms), inputPointers,
                        outputLocations);
}

// used by the C API (array of handles)
void multi_forward_handles(int n, Transform** ts, SpfftProcessingUnitType* in, double** out,
                           SpfftScalingType* sc) {
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_forward<double>(v, in, out, sc);
}
void multi_backward_handles(int n, Transform** ts, double** in, SpfftProcessingUnitType* out) {
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_backward<double>(v, in, out);
}
void multi_apply_local_handles(int n, Transform** ts, const double* const* in,
                               const double* const* pot, double* const* out,
                               const SpfftScalingType* sc) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_apply_local<double>(v, in, pot, out, sc);
}
void multi_apply_local_handles(int n, TransformFloat** ts, const float* const* in,
                               const float* const* pot, float* const* out,
                               const SpfftScalingType* sc) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_apply_local<float>(v, in, pot, out, sc);
}
void multi_accumulate_density_handles(int n, Transform** ts, const double* const* in,
                                      const double* weights, double* density) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_accumulate_density<double>(v, in, weights, density);
}
void multi_accumulate_density_handles(int n, TransformFloat** ts, const float* const* in,
                                      const float* weights, float* density) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_accumulate_density<float>(v, in, weights, density);
}
void multi_accumulate_fock_handles(int n, Transform** ts, const double* const* a, const double* const* b,
                                   const double* const* kernels, bool complexKernel, const double* weights,
                                   double* acc, SpfftScalingType scaling) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_accumulate_fock<double>(v, a, b, kernels, complexKernel, weights, acc, scaling);
}
void multi_accumulate_fock_handles(int n, TransformFloat** ts, const float* const* a, const float* const* b,
                                   const float* const* kernels, bool complexKernel, const float* weights,
                                   float* acc, SpfftScalingType scaling) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_accumulate_fock<float>(v, a, b, kernels, complexKernel, weights, acc, scaling);
}
void multi_reciprocal_fan_out_handles(int n, Transform** ts, SpfftProcessingUnitType location,
                                      const double* const* kernels, bool complexKernel, double* values,
                                      SpfftScalingType scaling) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_reciprocal_fan_out<double>(v, location, kernels, complexKernel, values, scaling);
}
void multi_reciprocal_fan_out_handles(int n, TransformFloat** ts, SpfftProcessingUnitType location,
                                      const float* const* kernels, bool complexKernel, float* values,
                                      SpfftScalingType scaling) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_reciprocal_fan_out<float>(v, location, kernels, complexKernel, values, scaling);
}
void multi_reciprocal_fan_in_handles(int n, Transform** ts, SpfftProcessingUnitType location,
                                     const double* const* kernels, bool complexKernel,
                                     SpfftScalingType scaling) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_reciprocal_fan_in<double>(v, location, kernels, complexKernel, scaling);
}
void multi_reciprocal_fan_in_handles(int n, TransformFloat** ts, SpfftProcessingUnitType location,
                                     const float* const* kernels, bool complexKernel,
                                     SpfftScalingType scaling) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_reciprocal_fan_in<float>(v, location, kernels, complexKernel, scaling);
}
void multi_accumulate_density_fan_handles(int n, Transform** ts, const double* input,
                                          const double* const* kernels, bool complexKernel,
                                          const double* weights, double* density) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_accumulate_density_fan<double>(v, input, kernels, complexKernel, weights, density);
}
void multi_accumulate_density_fan_handles(int n, TransformFloat** ts, const float* input,
                                          const float* const* kernels, bool complexKernel,
                                          const float* weights, float* density) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_accumulate_density_fan<float>(v, input, kernels, complexKernel, weights, density);
}
void multi_apply_local_fan_handles(int n, Transform** ts, const double* input, const double* const* kernelsIn,
                                   const double* const* potentials, const double* const* kernelsOut,
                                   bool complexKernel, double* output, SpfftScalingType scaling) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_apply_local_fan<double>(v, input, kernelsIn, potentials, kernelsOut, complexKernel, output, scaling);
}
void multi_apply_local_fan_handles(int n, TransformFloat** ts, const float* input, const float* const* kernelsIn,
                                   const float* const* potentials, const float* const* kernelsOut,
                                   bool complexKernel, float* output, SpfftScalingType scaling) {
  if (n < 0 || (n > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_apply_local_fan<float>(v, input, kernelsIn, potentials, kernelsOut, complexKernel, output, scaling);
}
void multi_apply_local_spinor_handles(int nSpinors, Transform** ts, const double* const* inputs,
                                       const double* const* potential, double* const* outputs,
                                       SpfftScalingType scaling) {
  if (nSpinors < 0 || (nSpinors > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < 2 * nSpinors; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_apply_local_spinor<double>(v, inputs, potential, outputs, scaling);
}
void multi_apply_local_spinor_handles(int nSpinors, TransformFloat** ts, const float* const* inputs,
                                       const float* const* potential, float* const* outputs,
                                       SpfftScalingType scaling) {
  if (nSpinors < 0 || (nSpinors > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < 2 * nSpinors; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_apply_local_spinor<float>(v, inputs, potential, outputs, scaling);
}
void multi_accumulate_spin_density_handles(int nSpinors, Transform** ts, const double* const* inputs,
                                            const double* weights, double* const* density) {
  if (nSpinors < 0 || (nSpinors > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<double>*> v;
  for (int i = 0; i < 2 * nSpinors; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_accumulate_spin_density<double>(v, inputs, weights, density);
}
void multi_accumulate_spin_density_handles(int nSpinors, TransformFloat** ts, const float* const* inputs,
                                            const float* weights, float* const* density) {
  if (nSpinors < 0 || (nSpinors > 0 && !ts)) throw InvalidParameterError();
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < 2 * nSpinors; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_accumulate_spin_density<float>(v, inputs, weights, density);
}
void multi_forward_handles(int n, TransformFloat** ts, SpfftProcessingUnitType* in, float** out,
                           SpfftScalingType* sc) {
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_forward<float>(v, in, out, sc);
}
void multi_backward_handles(int n, TransformFloat** ts, float** in, SpfftProcessingUnitType* out) {
  std::vector<TransformImpl<float>*> v;
  for (int i = 0; i < n; ++i) v.push_back(ts[i] ? ts[i]->impl().get() : nullptr);
  multi_backward<float>(v, in, out);
}

}  // namespace spfft
