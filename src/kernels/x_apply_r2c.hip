// Fused local-operator x stage on packed-real rows (R2C transforms with a
// compile-time half-length engine), fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template bool x_r2c_fused_fits<double>(int);
template void launch_x_apply_r2c<double>(const XArgs&, const double*, cx<double>*, bool, const cx<double>*,
                                         const cx<double>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
