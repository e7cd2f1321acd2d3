// Value fan-out and fan-in z stages and the composed value fan's plain add of
// the sparse values, fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_z_values_fan_out<float>(const ZArgs&, bool, const cx<float>*, const cx<float>*, hipStream_t);
template void launch_z_values_fan_in<float>(const ZArgs&, bool, cx<float>*, float, const cx<float>*, hipStream_t);
template void launch_values_add<float>(cx<float>*, const cx<float>*, long long, hipStream_t);

}  // namespace dev
}  // namespace spfft
