// Reciprocal fan-out and fan-in z stages and the composed fan-in path's
// multiply-add of the sparse values, fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template bool z_reciprocal_fan_fits<float>(const ZArgs&);
template void launch_z_reciprocal_fan_out<float>(const ZArgs&, bool, cx<float>*, float, const cx<float>*,
                                                 hipStream_t);
template void launch_z_reciprocal_fan_in<float>(const ZArgs&, bool, float, const cx<float>*, hipStream_t);
template void launch_values_scale_add<float>(cx<float>*, const cx<float>*, const float*, bool, long long,
                                             hipStream_t);

}  // namespace dev
}  // namespace spfft
