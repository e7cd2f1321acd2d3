// Exchange pair operator x stages (forward: rows conj(a) * b; backward: acc += w a u
// from LDS) and the composed path's two one-pass space-domain kernels, fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_forward_pair<float>(const XArgs&, const cx<float>*, const cx<float>*, cx<float>*,
                                           const cx<float>*, hipStream_t);
template void launch_x_backward_fock<float>(const XArgs&, const cx<float>*, const cx<float>*, cx<float>*, float,
                                            const cx<float>*, hipStream_t);
template void launch_space_pair<float>(void*, const float*, const float*, long long, bool, hipStream_t);
template void launch_space_fock<float>(const void*, const float*, float*, float, long long, bool, hipStream_t);

}  // namespace dev
}  // namespace spfft
