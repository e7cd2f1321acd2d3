// Batched fused reciprocal-space operator z stage (the members of a batched pair
// operator over blockIdx.z, each with its own stick array and kernel K), fp64
// transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_z_reciprocal_batch<double>(const ZArgs&, bool, double, const cx<double>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
