// Spinor x stages and the composed spinor paths' passes over two space
// domains, fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template bool x_spinor_fits<float>(int);
template void launch_x_spinor_apply<float>(const XArgs&, int, cx<float>* const*, cx<float>* const*,
                                           const float* const*, bool, const cx<float>*, hipStream_t);
template void launch_x_spinor_density<float>(const XArgs&, int, const cx<float>* const*, const cx<float>* const*,
                                             const float*, float* const*, const cx<float>*, hipStream_t);
template void launch_space_spinor_mix<float>(cx<float>*, cx<float>*, const float* const*, long long,
                                             hipStream_t);
template void launch_space_spin_density<float>(const cx<float>*, const cx<float>*, float* const*, float,
                                               long long, hipStream_t);

}  // namespace dev
}  // namespace spfft
