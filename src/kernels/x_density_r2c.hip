// Fused density x stage on packed-real rows (R2C transforms with a compile-time
// half-length engine), fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_density_r2c<double>(const XArgs&, const cx<double>*, double*, const double*, const cx<double>*,
                                           const cx<double>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
