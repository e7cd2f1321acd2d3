// Fused density x stage on packed-real rows (R2C transforms with a compile-time
// half-length engine), fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_density_r2c<float>(const XArgs&, const cx<float>*, float*, const float*, const cx<float>*,
                                           const cx<float>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
