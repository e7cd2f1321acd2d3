// Pair operator (Fock) x stages on packed-real rows (R2C transforms with a
// compile-time half-length engine), single and batched, fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template bool x_r2c_fock_fits<double>(int);
template void launch_x_forward_pair_r2c<double>(const XArgs&, const double*, const double*, cx<double>*, const cx<double>*,
                                         const cx<double>*, hipStream_t);
template void launch_x_backward_fock_r2c<double>(const XArgs&, const cx<double>*, const double*, double*, double, const cx<double>*,
                                          const cx<double>*, hipStream_t);
template void launch_x_forward_pair_r2c_batch<double>(const XArgs&, const double* const*, bool, const cx<double>*,
                                               const cx<double>*, hipStream_t);
template void launch_x_backward_fock_r2c_batch<double>(const XArgs&, const double* const*, const double*, double*,
                                                const cx<double>*, const cx<double>*, hipStream_t);

}  // namespace dev
}  // namespace spfft
