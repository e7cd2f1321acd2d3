// Batched exchange pair operator x stages (forward: the members over blockIdx.z;
// backward: the member loop inside the workgroup that owns the tile of acc),
// fp32 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_forward_pair_batch<float>(const XArgs&, const cx<float>* const*, bool, const cx<float>*,
                                                 hipStream_t);
template void launch_x_backward_fock_batch<float>(const XArgs&, const cx<float>* const*, const float*, cx<float>*,
                                                  const cx<float>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
