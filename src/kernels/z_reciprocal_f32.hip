// Fused reciprocal-space operator z stage and the composed path's multiply of
// the sparse values, fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_z_reciprocal<float>(const ZArgs&, cx<float>*, const float*, bool, cx<float>*, float,
                                         const cx<float>*, hipStream_t);
template void launch_values_scale<float>(cx<float>*, const cx<float>*, const float*, bool, long long, hipStream_t);

}  // namespace dev
}  // namespace spfft
