// Pair operator (Fock) x stages on packed-real rows (R2C transforms with a
// compile-time half-length engine), single and batched, fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template bool x_r2c_fock_fits<float>(int);
template void launch_x_forward_pair_r2c<float>(const XArgs&, const float*, const float*, cx<float>*, const cx<float>*,
                                         const cx<float>*, hipStream_t);
template void launch_x_backward_fock_r2c<float>(const XArgs&, const cx<float>*, const float*, float*, float, const cx<float>*,
                                          const cx<float>*, hipStream_t);
template void launch_x_forward_pair_r2c_batch<float>(const XArgs&, const float* const*, bool, const cx<float>*,
                                               const cx<float>*, hipStream_t);
template void launch_x_backward_fock_r2c_batch<float>(const XArgs&, const float* const*, const float*, float*,
                                                const cx<float>*, const cx<float>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
