// TransformImpl<T>: validated plan + executor (reference: src/spfft/transform_internal.{hpp,cpp}).
#pragma once

#include <memory>
#include <vector>

#include "api/grid_impl.hpp"
#include "gpu/gpu_executor.hpp"
#include "host/host_executor.hpp"
#include "plan/index_plan.hpp"

namespace spfft {

template <typename T>
class TransformImpl {
public:
  TransformImpl(std::shared_ptr<GridImpl<T>> grid, SpfftProcessingUnitType executionUnit,
                SpfftTransformType type, int dimX, int dimY, int dimZ, int localZLength,
                int numLocalElements, SpfftIndexFormatType format, const int* indices);
  TransformImpl(std::shared_ptr<GridImpl<T>> grid, SpfftProcessingUnitType executionUnit,
                std::shared_ptr<const IndexPlan> plan);

  std::shared_ptr<TransformImpl> clone() const;

  void forward(SpfftProcessingUnitType inputLocation, T* output, SpfftScalingType scaling);
  void backward(const T* input, SpfftProcessingUnitType outputLocation);

  // output = forward(V * backward(input)) with the real potential V over the
  // local space domain [localZ][dimY][dimX]; the space domain's contents are
  // unspecified afterwards (untouched on the fused GPU path)
  void apply_local(const T* input, const T* potential, T* output, SpfftScalingType scaling);
  bool apply_local_fused() const { return gpu_ && gpu_->apply_local_fused(); }
  // the stage between the two exchanges of apply_local (multi-transform interleaving)
  void apply_local_xy(const T* potential);

  // density[z][y][x] += weight * |backward(input)[z][y][x]|^2 over the local
  // space domain (R2C: weight * s^2); density is updated in place, input is not
  // modified, the space domain's contents are unspecified afterwards (untouched
  // on the fused GPU path)
  void accumulate_density(const T* input, T weight, T* density);
  bool density_fused() const { return gpu_ && gpu_->density_fused(); }
  // the stage behind backward_exchange (multi-transform interleaving)
  void accumulate_density_xy(T* density, T weight);

  // space domain = backward(K * (scale * forward(space domain))) with one real or
  // complex (interleaved) entry of K per local frequency value, in the order of
  // the transform's index triplets. `values` (may be NULL) receives the scaled
  // forward values before the multiply. `location` is where the input space
  // domain is read and the output space domain is written.
  void apply_reciprocal(SpfftProcessingUnitType location, const T* kernel, bool complexKernel,
                        T* values, SpfftScalingType scaling);
  bool reciprocal_fused() const { return gpu_ && gpu_->reciprocal_fused(); }
  // whether this transform and n - 1 clones of it, called with device pointers,
  // run the fused z stage of multi_transform_reciprocal_fan_out / fan_in (n == 1:
  // that of apply_reciprocal)
  bool reciprocal_fan_fused(int n) const;
  // whether this transform and n - 1 clones of it, called with device pointers,
  // run the fused z fan stages of multi_transform_accumulate_density_fan /
  // multi_transform_apply_local_fan
  bool values_fan_fused(int n) const;
  // whether this transform and a clone of it, called with device pointers, run
  // the fused x stages of multi_transform_apply_local_spinor /
  // multi_transform_accumulate_spin_density
  bool spinor_fused() const { return gpu_ && gpu_->spinor_fused(); }

  // Exchange (Fock) pair operator: acc += weight * a * backward(K * (scale *
  // forward(conj(a) * b))) with a, b and acc over the local space domain
  // [localZ][dimY][dimX] (interleaved complex; real for R2C, where conj is the
  // identity). kernel and values as in apply_reciprocal. a and b are not
  // modified (a == b is allowed); the space domain's contents are unspecified
  // afterwards (untouched on the fused GPU path).
  void accumulate_fock(const T* a, const T* b, const T* kernel, bool complexKernel, T weight, T* acc,
                       T* values, SpfftScalingType scaling);
  bool fock_fused() const { return gpu_ && gpu_->fock_fused(); }
  bool fock_r2c_fused() const { return gpu_ && gpu_->fock_r2c_fused(); }
  // the stages of accumulate_fock around the two exchanges (multi-transform
  // interleaving): fock_forward_xy, forward_exchange, reciprocal_z,
  // backward_exchange, fock_backward_xy
  void fock_forward_xy(const T* a, const T* b);
  void reciprocal_z(const T* kernel, bool complexKernel, T* values, SpfftScalingType scaling);
  void fock_backward_xy(const T* a, T* acc, T weight);

  void forward_xy(SpfftProcessingUnitType inputLocation);
  void forward_exchange(bool nonBlocking);
  void forward_z(T* output, SpfftScalingType scaling);
  void backward_z(const T* input);
  void backward_exchange(bool nonBlocking);
  void backward_xy(SpfftProcessingUnitType outputLocation);
  void synchronize();
  void set_stream(void* stream, bool synchronous);
  void reset_stream();

  T* space_domain_data(SpfftProcessingUnitType location);

  const IndexPlan& plan() const { return *plan_; }
  const std::shared_ptr<GridImpl<T>>& grid() const { return grid_; }
  SpfftProcessingUnitType processing_unit() const { return exec_; }
  bool is_gpu() const { return static_cast<bool>(gpu_); }
  GpuExecutor<T>* gpu() { return gpu_.get(); }

private:
  void create_executor();

  std::shared_ptr<GridImpl<T>> grid_;
  SpfftProcessingUnitType exec_;
  std::shared_ptr<const IndexPlan> plan_;
  std::unique_ptr<HostExecutor<T>> host_;
  std::unique_ptr<GpuExecutor<T>> gpu_;
  std::vector<T> reciprocalWork_;  // host apply_reciprocal: the frequency values
};

}  // namespace spfft
