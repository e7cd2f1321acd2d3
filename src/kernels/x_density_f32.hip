// Fused density x stage (inverse x FFT in LDS, rho += w |psi|^2) and the composed
// path's one-pass space-domain kernel, fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_density<float>(const XArgs&, const cx<float>*, float*, const float*, const cx<float>*,
                                    hipStream_t);
template void launch_space_density<float>(const void*, float*, float, long long, bool, hipStream_t);

}  // namespace dev
}  // namespace spfft
