// Fused reciprocal-space operator z stage (forward z FFT, K(G) multiply,
// inverse z FFT in LDS) and the composed path's multiply of the sparse values,
// fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_z_reciprocal<double>(const ZArgs&, cx<double>*, const double*, bool, cx<double>*, double,
                                          const cx<double>*, hipStream_t);
template void launch_values_scale<double>(cx<double>*, const cx<double>*, const double*, bool, long long, hipStream_t);

}  // namespace dev
}  // namespace spfft
