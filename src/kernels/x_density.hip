// Fused density x stage (inverse x FFT in LDS, rho += w |psi|^2) and the composed
// path's one-pass space-domain kernel, fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_density<double>(const XArgs&, const cx<double>*, double*, const double*, const cx<double>*,
                                    hipStream_t);
template void launch_space_density<double>(const void*, double*, double, long long, bool, hipStream_t);

}  // namespace dev
}  // namespace spfft
