// Fused local-operator x stage (inverse x FFT, V(r) multiply, forward x FFT in
// LDS) and the unfused path's space-domain multiply, fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_apply<double>(const XArgs&, const double*, cx<double>*, bool, const cx<double>*,
                                     hipStream_t);
template void launch_space_scale<double>(void*, const double*, long long, bool, hipStream_t);

}  // namespace dev
}  // namespace spfft
