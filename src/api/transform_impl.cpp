#include "api/transform_impl.hpp"

#include <algorithm>

#include "core/timing.hpp"
#include "spfft/exceptions.hpp"

namespace spfft {

namespace {
template <typename T>
void check_against_grid(const GridImpl<T>& g, SpfftProcessingUnitType exec, int dimX, int dimY,
                        int dimZ) {
  // reference: src/spfft/transform_internal.cpp:52-77
  if (dimX > g.max_dim_x() || dimY > g.max_dim_y() || dimZ > g.max_dim_z())
    throw InvalidParameterError();
  if (!(exec & g.processing_unit())) throw InvalidParameterError();
  if (exec != SPFFT_PU_HOST && exec != SPFFT_PU_GPU) throw InvalidParameterError();
}
}  // namespace

template <typename T>
TransformImpl<T>::TransformImpl(std::shared_ptr<GridImpl<T>> grid,
                                SpfftProcessingUnitType executionUnit, SpfftTransformType type,
                                int dimX, int dimY, int dimZ, int localZLength,
                                int numLocalElements, SpfftIndexFormatType format,
                                const int* indices)
    : grid_(std::move(grid)), exec_(executionUnit) {
  if (!grid_) throw InvalidParameterError();
  if (dimX < 0 || dimY < 0 || dimZ < 0 || localZLength < 0 || numLocalElements < 0 ||
      (!indices && numLocalElements > 0))
    throw InvalidParameterError();
  // Purely local checks may throw before any collective; the distributed plan
  // construction reports errors to every rank (plan/index_plan.cpp).
  if (grid_->local()) check_against_grid(*grid_, exec_, dimX, dimY, dimZ);
  plan_ = std::make_shared<const IndexPlan>(grid_->local() ? nullptr : grid_->communicator().get(),
                                            type, dimX, dimY, dimZ, localZLength,
                                            numLocalElements, format, indices);
  check_against_grid(*grid_, exec_, dimX, dimY, dimZ);
  if (plan_->local_planes() > grid_->max_local_z_length()) throw InvalidParameterError();
  if (plan_->local_sticks() > grid_->max_num_local_z_columns()) throw InvalidParameterError();
  create_executor();
}

template <typename T>
TransformImpl<T>::TransformImpl(std::shared_ptr<GridImpl<T>> grid,
                                SpfftProcessingUnitType executionUnit,
                                std::shared_ptr<const IndexPlan> plan)
    : grid_(std::move(grid)), exec_(executionUnit), plan_(std::move(plan)) {
  create_executor();
}

template <typename T>
void TransformImpl<T>::create_executor() {
  if (exec_ == SPFFT_PU_HOST)
    host_.reset(new HostExecutor<T>(grid_, plan_));
  else
    gpu_.reset(new GpuExecutor<T>(grid_, plan_));
}

template <typename T>
std::shared_ptr<TransformImpl<T>> TransformImpl<T>::clone() const {
  auto newGrid = std::make_shared<GridImpl<T>>(*grid_);
  return std::make_shared<TransformImpl<T>>(newGrid, exec_, plan_);
}

template <typename T>
T* TransformImpl<T>::space_domain_data(SpfftProcessingUnitType location) {
  if (exec_ == SPFFT_PU_HOST) {
    if (location != SPFFT_PU_HOST) throw InvalidParameterError();
    return host_->space_domain();
  }
  return gpu_->space_domain(location);
}

template <typename T>
void TransformImpl<T>::forward(SpfftProcessingUnitType inputLocation, T* output,
                               SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("forward");
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  if (gpu_ && gpu_->forward_graph(inputLocation, output, scaling)) {
    if (gpu_->synchronous()) gpu_->synchronize();
    return;
  }
  forward_xy(inputLocation);
  forward_exchange(false);
  forward_z(output, scaling);
  if (gpu_ && gpu_->synchronous()) gpu_->synchronize();
}

template <typename T>
void TransformImpl<T>::backward(const T* input, SpfftProcessingUnitType outputLocation) {
  SPFFT_TIMED_SCOPE("backward");
  if (gpu_ && gpu_->backward_graph(input, outputLocation)) {
    if (gpu_->synchronous()) gpu_->synchronize();
    return;
  }
  backward_z(input);
  backward_exchange(false);
  backward_xy(outputLocation);
  if (gpu_ && gpu_->synchronous()) gpu_->synchronize();
}

template <typename T>
void TransformImpl<T>::apply_local(const T* input, const T* potential, T* output,
                                   SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("apply_local");
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  if (!potential && plan_->local_planes() > 0) throw InvalidParameterError();
  backward_z(input);
  backward_exchange(false);
  apply_local_xy(potential);
  forward_exchange(false);
  forward_z(output, scaling);
  if (gpu_ && gpu_->synchronous()) gpu_->synchronize();
}

template <typename T>
void TransformImpl<T>::apply_local_xy(const T* potential) {
  // (a rank without planes has an empty space domain and may pass no potential)
  if (!potential && plan_->local_planes() > 0) throw InvalidParameterError();
  if (gpu_) {
    gpu_->apply_local_xy(potential);
    return;
  }
  // host: the plain composition through the space domain
  host_->backward_xy();
  const IndexPlan& p = *plan_;
  const std::size_t count = static_cast<std::size_t>(p.local_planes()) * p.dimY * p.dimX;
  T* space = host_->space_domain();
  if (p.type == SPFFT_TRANS_R2C) {
    for (std::size_t i = 0; i < count; ++i) space[i] *= potential[i];
  } else {
    for (std::size_t i = 0; i < count; ++i) {
      space[2 * i] *= potential[i];
      space[2 * i + 1] *= potential[i];
    }
  }
  host_->forward_xy();
}

template <typename T>
void TransformImpl<T>::accumulate_density(const T* input, T weight, T* density) {
  SPFFT_TIMED_SCOPE("accumulate_density");
  if (!density && plan_->local_planes() > 0) throw InvalidParameterError();
  backward_z(input);
  backward_exchange(false);
  accumulate_density_xy(density, weight);
  if (gpu_ && gpu_->synchronous()) gpu_->synchronize();
}

template <typename T>
void TransformImpl<T>::accumulate_density_xy(T* density, T weight) {
  const IndexPlan& p = *plan_;
  if (!density && p.local_planes() > 0) throw InvalidParameterError();
  if (gpu_) {
    gpu_->accumulate_density_xy(density, weight);
    return;
  }
  // host: the plain composition through the space domain
  host_->backward_xy();
  const std::size_t count = static_cast<std::size_t>(p.local_planes()) * p.dimY * p.dimX;
  const T* space = host_->space_domain();
  if (p.type == SPFFT_TRANS_R2C) {
    for (std::size_t i = 0; i < count; ++i) density[i] += weight * (space[i] * space[i]);
  } else {
    for (std::size_t i = 0; i < count; ++i)
      density[i] += weight * (space[2 * i] * space[2 * i] + space[2 * i + 1] * space[2 * i + 1]);
  }
}

template <typename T>
void TransformImpl<T>::apply_reciprocal(SpfftProcessingUnitType location, const T* kernel,
                                        bool complexKernel, T* values, SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("apply_reciprocal");
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  if (location != SPFFT_PU_HOST && location != SPFFT_PU_GPU) throw InvalidParameterError();
  if (host_ && location != SPFFT_PU_HOST) throw InvalidParameterError();
  const std::size_t count = static_cast<std::size_t>(plan_->numLocalElements);
  if (!kernel && count > 0) throw InvalidParameterError();
  forward_xy(location);
  forward_exchange(false);
  reciprocal_z(kernel, complexKernel, values, scaling);
  backward_exchange(false);
  backward_xy(location);
  if (gpu_ && gpu_->synchronous()) gpu_->synchronize();
}

// the stage between the two exchanges of apply_reciprocal and accumulate_fock
template <typename T>
void TransformImpl<T>::reciprocal_z(const T* kernel, bool complexKernel, T* values,
                                    SpfftScalingType scaling) {
  const std::size_t count = static_cast<std::size_t>(plan_->numLocalElements);
  if (gpu_) {
    gpu_->reciprocal_z(kernel, complexKernel, values, scaling);
  } else {
    // host: the plain composition through the frequency values
    std::vector<T>& work = reciprocalWork_;
    work.resize(2 * std::max<std::size_t>(count, 1));
    host_->forward_z(work.data(), scaling);
    if (values) std::copy(work.begin(), work.begin() + 2 * count, values);
    if (complexKernel) {
      for (std::size_t i = 0; i < count; ++i) {
        const T re = work[2 * i], im = work[2 * i + 1];
        work[2 * i] = re * kernel[2 * i] - im * kernel[2 * i + 1];
        work[2 * i + 1] = re * kernel[2 * i + 1] + im * kernel[2 * i];
      }
    } else {
      for (std::size_t i = 0; i < count; ++i) {
        work[2 * i] *= kernel[i];
        work[2 * i + 1] *= kernel[i];
      }
    }
    host_->backward_z(work.data());
  }
}

template <typename T>
void TransformImpl<T>::accumulate_fock(const T* a, const T* b, const T* kernel, bool complexKernel,
                                       T weight, T* acc, T* values, SpfftScalingType scaling) {
  SPFFT_TIMED_SCOPE("accumulate_fock");
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  const IndexPlan& p = *plan_;
  const std::size_t space = static_cast<std::size_t>(p.local_planes()) * p.dimY * p.dimX;
  if (space > 0 && (!a || !b || !acc)) throw InvalidParameterError();
  if (!kernel && p.numLocalElements > 0) throw InvalidParameterError();
  fock_forward_xy(a, b);
  forward_exchange(false);
  reciprocal_z(kernel, complexKernel, values, scaling);
  backward_exchange(false);
  fock_backward_xy(a, acc, weight);
  if (gpu_ && gpu_->synchronous()) gpu_->synchronize();
}

// the stages of accumulate_fock in front of forward_exchange and behind
// backward_exchange (multi-transform interleaving)
template <typename T>
void TransformImpl<T>::fock_forward_xy(const T* a, const T* b) {
  if (gpu_) {
    gpu_->fock_forward_xy(a, b);
    return;
  }
  // host: the plain composition through the space domain
  const IndexPlan& p = *plan_;
  const std::size_t space = static_cast<std::size_t>(p.local_planes()) * p.dimY * p.dimX;
  T* s = host_->space_domain();
  if (p.type == SPFFT_TRANS_R2C) {
    for (std::size_t i = 0; i < space; ++i) s[i] = a[i] * b[i];
  } else {
    for (std::size_t i = 0; i < space; ++i) {
      const T ar = a[2 * i], ai = a[2 * i + 1], br = b[2 * i], bi = b[2 * i + 1];
      s[2 * i] = ar * br + ai * bi;
      s[2 * i + 1] = ar * bi - ai * br;
    }
  }
  host_->forward_xy();
}

template <typename T>
void TransformImpl<T>::fock_backward_xy(const T* a, T* acc, T weight) {
  if (gpu_) {
    gpu_->fock_backward_xy(a, acc, weight);
    return;
  }
  const IndexPlan& p = *plan_;
  const std::size_t space = static_cast<std::size_t>(p.local_planes()) * p.dimY * p.dimX;
  host_->backward_xy();
  const T* u = host_->space_domain();
  if (p.type == SPFFT_TRANS_R2C) {
    for (std::size_t i = 0; i < space; ++i) acc[i] += weight * a[i] * u[i];
  } else {
    for (std::size_t i = 0; i < space; ++i) {
      const T tr = weight * a[2 * i], ti = weight * a[2 * i + 1];
      acc[2 * i] += tr * u[2 * i] - ti * u[2 * i + 1];
      acc[2 * i + 1] += tr * u[2 * i + 1] + ti * u[2 * i];
    }
  }
}

template <typename T>
void TransformImpl<T>::forward_xy(SpfftProcessingUnitType inputLocation) {
  if (host_) {
    if (inputLocation != SPFFT_PU_HOST) throw InvalidParameterError();
    host_->forward_xy();
  } else {
    gpu_->forward_xy(inputLocation);
  }
}

template <typename T>
void TransformImpl<T>::forward_exchange(bool nonBlocking) {
  if (host_)
    host_->forward_exchange(nonBlocking);
  else
    gpu_->forward_exchange(nonBlocking);
}

template <typename T>
void TransformImpl<T>::forward_z(T* output, SpfftScalingType scaling) {
  if (scaling != SPFFT_NO_SCALING && scaling != SPFFT_FULL_SCALING) throw InvalidParameterError();
  if (host_)
    host_->forward_z(output, scaling);
  else
    gpu_->forward_z(output, scaling);
}

template <typename T>
void TransformImpl<T>::backward_z(const T* input) {
  if (host_)
    host_->backward_z(input);
  else
    gpu_->backward_z(input);
}

template <typename T>
void TransformImpl<T>::backward_exchange(bool nonBlocking) {
  if (host_)
    host_->backward_exchange(nonBlocking);
  else
    gpu_->backward_exchange(nonBlocking);
}

template <typename T>
void TransformImpl<T>::backward_xy(SpfftProcessingUnitType outputLocation) {
  if (host_) {
    if (outputLocation != SPFFT_PU_HOST) throw InvalidParameterError();
    host_->backward_xy();
  } else {
    gpu_->backward_xy(outputLocation);
  }
}

template <typename T>
bool TransformImpl<T>::reciprocal_fan_fused(int n) const {
  if (!gpu_ || n < 1 || n > dev::kMaxBatch) return false;
  return n == 1 ? gpu_->reciprocal_fused() : gpu_->reciprocal_fan_fused();
}

template <typename T>
bool TransformImpl<T>::values_fan_fused(int n) const {
  return gpu_ && n >= 1 && n <= dev::kMaxBatch && gpu_->values_fan_fused();
}

template <typename T>
void TransformImpl<T>::synchronize() {
  if (gpu_) gpu_->synchronize();
}

template <typename T>
void TransformImpl<T>::set_stream(void* stream, bool synchronous) {
  if (!gpu_) throw InvalidParameterError();
  gpu_->set_stream(static_cast<hipStream_t>(stream), synchronous);
}

template <typename T>
void TransformImpl<T>::reset_stream() {
  if (!gpu_) throw InvalidParameterError();
  gpu_->reset_stream();
}

template class TransformImpl<double>;
template class TransformImpl<float>;

}  // namespace spfft
