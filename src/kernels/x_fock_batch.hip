// Batched exchange pair operator x stages (forward: the members over blockIdx.z;
// backward: the member loop inside the workgroup that owns the tile of acc),
// fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_forward_pair_batch<double>(const XArgs&, const cx<double>* const*, bool, const cx<double>*,
                                                  hipStream_t);
template void launch_x_backward_fock_batch<double>(const XArgs&, const cx<double>* const*, const double*,
                                                   cx<double>*, const cx<double>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
