// Value fan-out and fan-in z stages (one set of frequency values feeding an
// inverse z FFT per member; the members' coefficients summed into one set of
// values) and the composed value fan's plain add of the sparse values, fp64
// transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_z_values_fan_out<double>(const ZArgs&, bool, const cx<double>*, const cx<double>*,
                                              hipStream_t);
template void launch_z_values_fan_in<double>(const ZArgs&, bool, cx<double>*, double, const cx<double>*,
                                             hipStream_t);
template void launch_values_add<double>(cx<double>*, const cx<double>*, long long, hipStream_t);

}  // namespace dev
}  // namespace spfft
