// Reciprocal fan-out and fan-in z stages (one forward z FFT feeding an inverse
// z FFT per member; the members' coefficients summed in front of one inverse z
// FFT) and the composed fan-in path's multiply-add of the sparse values, fp64
// transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template bool z_reciprocal_fan_fits<double>(const ZArgs&);
template void launch_z_reciprocal_fan_out<double>(const ZArgs&, bool, cx<double>*, double, const cx<double>*,
                                                  hipStream_t);
template void launch_z_reciprocal_fan_in<double>(const ZArgs&, bool, double, const cx<double>*, hipStream_t);
template void launch_values_scale_add<double>(cx<double>*, const cx<double>*, const double*, bool, long long,
                                              hipStream_t);

}  // namespace dev
}  // namespace spfft
