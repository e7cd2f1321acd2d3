// Fused local-operator x stage and space-domain multiply, fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_apply<float>(const XArgs&, const float*, cx<float>*, bool, const cx<float>*,
                                    hipStream_t);
template void launch_space_scale<float>(void*, const float*, long long, bool, hipStream_t);

}  // namespace dev
}  // namespace spfft
