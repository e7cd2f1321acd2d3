// Fused local-operator x stage on packed-real rows (R2C transforms with a
// compile-time half-length engine), fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template bool x_r2c_fused_fits<float>(int);
template void launch_x_apply_r2c<float>(const XArgs&, const float*, cx<float>*, bool, const cx<float>*,
                                         const cx<float>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
